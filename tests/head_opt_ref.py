"""
Plain torch restatements of the entry points of csrc/head_opt.hip, written from the contract in include/ecgvit_hip.h (not from the kernels),
with the case lists and input generators that tests/test_head_opt_ref.py (CPU) and tests/test_gpu_head_opt.py (MI355X) share.

Every restatement takes a `dtype`: in float64 it is the reference, in float32 it is the "plain f32 restatement" that calibrates the
tolerances.  Each returns (out, mag): two dicts name -> tensor.  mag[name] is the sum of the absolute values of the terms of the final
expression of out[name], in float64 (for a logit: sum_c |xn_c W_kc| + |bias_k|), floored at the smallest normal f32.  Errors are judged element
by element as

        ratio = |got - ref| / (u * mag),   u = 2^-24

(a bf16 output is first allowed half a bf16 ulp of the reference: 2^(e - 9) for 2^(e - 1) <= |ref| < 2^e, i.e. 2^-9 |ref| .. 2^-8 |ref|)

and never relative to |ref|: where an update cancels its parameter, or a sum cancels, an honest f32 result is thousands of u away relative to
|ref|.  The floor makes the tolerance of a result in the f32 denormal range C / 2 denormal quanta (u * 2^-126 = 2^-150): every output answers
for its denormal results (sigmoid(-89) = 2.2e-39 is one), so a build of the kernels that flushes f32 denormals to zero fails this suite.

The committed constants C[name] turn the unit into a tolerance: the GPU test asserts ratio <= C[name].  test_head_opt_ref.py proves, for every
case the GPU file runs, that (a) the plain f32 restatement's worst ratio is <= C / 4 (room for another summation order and a device expf /
log1pf a few ulp off libm's) and (b) every applicable perturbed reference (`perturb=`) lies >= 2 C away.

Measured ratios (worst over the case lists).  `f32` = the plain f32 restatement on the CPU, `perturbed` = the nearest applicable perturbed
reference (its name beside it), `MI355X` = the kernels of csrc/head_opt.hip:

    name                  C      f32   nearest perturbed reference                MI355X
    head_fwd.logits      16     2.75    9.37e+03 drop_last_term                   1.32
    head_fwd.xhat        24     4.41        75.1 eps_outside                      10.2
    head_fwd.rstd        16     2.35        75.1 eps_outside                      2.19
    head_bwd.dW          16     3.86    1.86e+05 drop_last_row                    3.18
    head_bwd.dbias       16     2.59    5.58e+04 drop_last_row                    1.24
    head_bwd.dgamma      16      1.8    5.54e+04 drop_last_row                    2.04
    head_bwd.dbeta       16     1.73    2.35e+04 drop_last_row                    1.69
    head_bwd.dX          16     2.52    2.63e+05 drop_last_term                   2.52
    bce_fwd.loss_elem    16     2.65    1.68e+07 drop_last_term                   2.77
    bce_fwd.loss_mean     8    0.891         460 drop_last_term                   0.752
    bce_bwd.dlogits      16     3.85    1.12e+07 drop_last_term                   3.47
    sumsq.out             8    0.949         294 drop_last_term                   2.39
    sumsq_spans.out       8    0.181         705 drop_last_term                   0.181
    adamw.p              32     5.37    1.69e+03 span_step_offset_ignored         4.87
    adamw.m              16     3.04    8.09e+06 coupled_for_decoupled            2.57
    adamw.v              32     5.41    3.97e+03 no_clip                          4.63
    adamw.norm            8    0.621           - (no perturbation applies)        0.654
    clip_scale.g          8      1.4     2.3e+09 no_clip                          1.41
    clip_scale.norm       8    0.455           - (no perturbation applies)        0.455
    adamw.trajectory20 (u (|p| + lr), bound 20 C[adamw.p] = 640): f32 38.9, MI355X 34.4

(the adamw rows hold the whole-buffer and the span kernels together: the span kernel alone reaches p 4.42, m 1.89, v 3.52, norm 0.654;
the whole-buffer kernel p 4.87, m 2.57, v 4.63, norm 0.621.)

The exact-integer families (head backward on small integers; sum of squares of values in {-2..2}, whole buffer and spans) are exact on the
MI355X: bit for bit the integer result.  scale = 1 accumulation, the transposes and both casts are bit-exact as well.

Where a perturbed reference coincides with the reference by construction it is not asked to lie 2 C away, and the test says so at the spot:
d = 1 (xhat, dgamma and dX are identically zero), the bias corrections at step - 1 for step = 1 and step >= 100 000, the other decay at wd = 0,
the clip coefficient where the clip is off or does not bind, a misplaced eps on the xhat of the mean-100 rows (held on rstd there).
"""
import math

import torch

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
EPS_LN = 1e-5


def f32r(x):
    """a Python scalar as the C ABI passes it: rounded to f32"""
    return float(torch.tensor(x, dtype=F32))


def _floor(m):
    return m.double().clamp_min(FLT_MIN)


def ratio(got, ref, mag, bf16_out=False):
    """worst |got - ref| / (u mag) over the elements; a bf16 output is first allowed half a bf16 ulp of the reference"""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    den = U * _floor(mag).reshape(-1)
    err = (got - ref).abs()
    if bf16_out:
        err = (err - torch.ldexp(torch.ones_like(ref), torch.frexp(ref).exponent - 9) * (ref != 0)).clamp_min(0)     # a zero reference has no ulp
    r = err / den
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return float(r.max())


# ===================================================================================================================== constants
# name -> C.  The measurements behind them are in the table of the module docstring.
C = {
    'head_fwd.logits': 16.0, 'head_fwd.xhat': 24.0, 'head_fwd.rstd': 16.0,
    'head_bwd.dW': 16.0, 'head_bwd.dbias': 16.0, 'head_bwd.dgamma': 16.0, 'head_bwd.dbeta': 16.0, 'head_bwd.dX': 16.0,
    'bce_fwd.loss_elem': 16.0, 'bce_fwd.loss_mean': 8.0, 'bce_bwd.dlogits': 16.0,
    'sumsq.out': 8.0, 'sumsq_spans.out': 8.0,
    'adamw.p': 32.0, 'adamw.m': 16.0, 'adamw.v': 32.0, 'adamw.norm': 8.0,
    'clip_scale.g': 8.0, 'clip_scale.norm': 8.0,
}


# ===================================================================================================================== restatements
def head_fwd(x_cls, gamma, beta, W, bias, eps=EPS_LN, dtype=F64, perturb=None):
    """logits[b,k] = LN(x_cls[b]) . W[k] + bias[k]; xhat, rstd saved for the backward.
    perturb: 'drop_last_term' (c = d - 1 left out of the product), 'eps_outside' (1 / (sqrt(var) + eps)), 'one_pass_var' (E[x^2] - mu^2)"""
    x, g, b, W, bias = (t.to(dtype) for t in (x_cls, gamma, beta, W, bias))
    eps = f32r(eps)
    mu = x.mean(1, keepdim=True)
    t = x - mu
    var = (t * t).mean(1, keepdim=True)
    if perturb == 'one_pass_var':
        var = (x * x).mean(1, keepdim=True) - mu * mu
    rstd = 1.0 / (var.sqrt() + eps) if perturb == 'eps_outside' else 1.0 / (var + eps).sqrt()
    xhat = t * rstd
    xn = xhat * g + b
    if perturb == 'drop_last_term':
        logits = xn[:, :-1] @ W[:, :-1].T + bias
    else:
        logits = xn @ W.T + bias
    out = dict(logits=logits, xhat=xhat, rstd=rstd[:, 0])
    mag = dict(logits=_floor(xn.double().abs() @ W.double().abs().T + bias.double().abs()),
               xhat=_floor((x.double().abs() + mu.double().abs()) * rstd.double()), rstd=_floor(rstd[:, 0]))
    return out, mag


def head_bwd(dl, xhat, rstd, gamma, beta, W, dtype=F64, perturb=None):
    """backward of head_fwd from the saved xhat [B,d], rstd [B]: dW, dbias, dgamma, dbeta and the CLS rows of dX.
    perturb: 'drop_last_row' (record B - 1 left out of the four parameter gradients), 'drop_last_term' (class K - 1 left out of dX)"""
    dl, xhat, rstd, g, b, W = (t.to(dtype) for t in (dl, xhat, rstd, gamma, beta, W))
    d = xhat.shape[1]
    xn = xhat * g + b
    dxn = dl @ W                                      # [B, d]
    dlp, xnp, dxnp, xhp = dl, xn, dxn, xhat
    if perturb == 'drop_last_row':
        dlp, xnp, dxnp, xhp = dl[:-1], xn[:-1], dxn[:-1], xhat[:-1]
    dW = dlp.T @ xnp
    dbias = dlp.sum(0)
    dgamma = (dxnp * xhp).sum(0)
    dbeta = dxnp.sum(0)
    gg = (dl[:, :-1] @ W[:-1] if perturb == 'drop_last_term' else dxn) * g
    c1 = gg.mean(1, keepdim=True)
    c2 = (gg * xhat).mean(1, keepdim=True)
    dX = rstd[:, None] * (gg - c1 - xhat * c2)
    A = lambda t: t.double().abs()
    adxn = A(dl) @ A(W)
    agg = adxn * A(g)
    mag = dict(dW=A(dl).T @ (A(xhat) * A(g) + A(b)), dbias=A(dl).sum(0), dgamma=(adxn * A(xhat)).sum(0), dbeta=adxn.sum(0),
               dX=A(rstd)[:, None] * (agg + agg.mean(1, keepdim=True) + A(xhat) * (agg * A(xhat)).mean(1, keepdim=True)))
    assert d == W.shape[1]
    return dict(dW=dW, dbias=dbias, dgamma=dgamma, dbeta=dbeta, dX=dX), {k: _floor(v) for k, v in mag.items()}


def bce_fwd(z, y, w=None, dtype=F64, perturb=None):
    """l = w (max(z,0) - z y + log1p(exp(-|z|))), mean(l).  perturb: 'drop_last_term' (no log1p term; the mean without its last element)"""
    z, y = z.to(dtype), y.to(dtype)
    w = torch.ones_like(z) if w is None else w.to(dtype)
    soft = torch.log1p(torch.exp(-z.abs()))
    le = w * (z.clamp_min(0) - z * y + (0 if perturb == 'drop_last_term' else soft))
    full = w * (z.clamp_min(0) - z * y + soft)
    mean = (full[:-1].sum() if perturb == 'drop_last_term' else full.sum()) / z.numel()
    ml = _floor(w.double().abs() * (z.double().clamp_min(0) + (z.double() * y.double()).abs() + soft.double()))
    return dict(loss_elem=le, loss_mean=mean.reshape(1)), dict(loss_elem=ml, loss_mean=_floor(ml.sum().reshape(1) / z.numel()))


def bce_bwd(z, y, w=None, gelem=None, gscalar=None, gscale=1.0, dtype=F64, perturb=None):
    """dlogits = upstream w (sigmoid(z) - y); upstream = gelem[i] gscale, or gscalar[0] gscale, or gscale.  perturb: 'drop_last_term' (no y)"""
    z, y = z.to(dtype), y.to(dtype)
    up = torch.ones_like(z) if gelem is None and gscalar is None else (gelem if gelem is not None else gscalar).to(dtype).expand_as(z)
    up = up * f32r(gscale)
    if w is not None:
        up = up * w.to(dtype)
    e = torch.exp(-z.abs())      # the overflow-free form: 1 / (1 + e^-z) for z >= 0, e^z / (1 + e^z) below
    sg = torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    dz = (sg - (0 if perturb == 'drop_last_term' else y)) * up
    return dict(dlogits=dz), dict(dlogits=_floor((sg.double() + y.double().abs()) * up.double().abs()))


def sumsq(g, dtype=F64, perturb=None):
    """sum of g^2.  perturb: 'drop_last_term'"""
    g = g.to(dtype)
    s = (g * g).sum() if perturb != 'drop_last_term' else (g[:-1] * g[:-1]).sum()
    return dict(out=s.reshape(1)), dict(out=_floor((g.double() * g.double()).sum().reshape(1)))


def span_index(spans):
    """flat element indices of a span table [(offset, count, step offset), ...], in table order"""
    return torch.cat([torch.arange(o, o + n) for o, n, _ in spans])


def sumsq_spans(g, spans, dtype=F64, perturb=None):
    return sumsq(g[span_index(spans)], dtype, perturb)


def clip_coef(ss, grad_scale, max_norm, dtype=F64):
    """(norm, coef) of the contract: norm = |grad_scale| sqrt(sumsq); coef = min(1, max_norm / (norm + 1e-6)), 1 if max_norm <= 0"""
    norm = ss.to(dtype).reshape(()).sqrt() * abs(f32r(grad_scale))
    if max_norm <= 0:
        return norm, torch.ones((), dtype=dtype)
    return norm, torch.clamp(f32r(max_norm) / (norm + f32r(1e-6)), max=1.0)


def adamw(p, g, m, v, ss, grad_scale=1.0, max_norm=1.0, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.1, step=1, decoupled=True, dtype=F64,
          perturb=None):
    """one clip + AdamW / Adam step on flat buffers; every scalar is the f32 the ABI carries, the bias corrections are formed in double.
    perturb: 'eps_inside' (sqrt(v / bc2 + eps)), 'bias_step_minus_1', 'coupled_for_decoupled' (the other decay), 'no_clip' (coef = 1)"""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (f32r(s) for s in (lr, b1, b2, eps, wd, grad_scale))
    norm, coef = clip_coef(ss, grad_scale, max_norm, dtype)
    if perturb == 'no_clip':
        coef = torch.ones((), dtype=dtype)
    if perturb == 'coupled_for_decoupled':
        decoupled = not decoupled
    st = step - 1 if perturb == 'bias_step_minus_1' else step
    bc1, bc2 = 1.0 - b1 ** st, 1.0 - b2 ** st
    gc = g * (coef * gs)
    mag_g = gc.double().abs()
    if decoupled:
        p1 = p * (1.0 - lr * wd)
    else:
        p1 = p
        gc = gc + wd * p
        mag_g = mag_g + (wd * p.double()).abs()
    m1 = b1 * m + (1.0 - b1) * gc
    v1 = b2 * v + (1.0 - b2) * gc * gc
    if dtype == F32:   # the scalars a plain f32 program would form
        bc1_, bc2s = f32r(bc1), f32r(math.sqrt(bc2))
    else:
        bc1_, bc2s = bc1, math.sqrt(bc2)
    denom = (v1 / bc2 + eps).sqrt() if perturb == 'eps_inside' else v1.sqrt() / bc2s + eps
    upd = (lr / bc1_) * (m1 / denom)
    out = dict(p=p1 - upd, m=m1, v=v1, norm=norm.reshape(1))
    mag_m = (b1 * m.double()).abs() + (1.0 - b1) * mag_g       # m' and g' are sums themselves: their terms count, not their values
    mag = dict(p=p1.double().abs() + (lr / bc1) * (mag_m / denom.double()), m=mag_m,
               v=b2 * v.double().abs() + (1.0 - b2) * mag_g * mag_g, norm=norm.double().abs().reshape(1))
    return out, {k: _floor(x) for k, x in mag.items()}


def adamw_spans(p, g, m, v, spans, ss, step=1, dtype=F64, perturb=None, **kw):
    """adamw restricted to the spans, span s at step + spans[s][2]; (out, mag) hold whole buffers, elements outside the spans are the inputs"""
    out = dict(p=p.to(dtype).clone(), m=m.to(dtype).clone(), v=v.to(dtype).clone())
    mag = {k: torch.full(p.shape, FLT_MIN, dtype=F64) for k in out}
    for o, n, so in spans:
        s = slice(o, o + n)
        r, rm = adamw(p[s], g[s], m[s], v[s], ss, step=step + so, dtype=dtype, perturb=perturb, **kw)
        for k in out:
            out[k][s], mag[k][s] = r[k], rm[k]
        out['norm'], mag['norm'] = r['norm'], rm['norm']
    return out, mag


def clip_scale(g, ss, max_norm, dtype=F64, perturb=None):
    """g *= coef in place.  perturb: 'no_clip'"""
    norm, coef = clip_coef(ss, 1.0, max_norm, dtype)
    if perturb == 'no_clip':
        coef = torch.ones((), dtype=dtype)
    r = g.to(dtype) * coef
    return dict(g=r, norm=norm.reshape(1)), dict(g=_floor(r.double().abs()), norm=_floor(norm.double().reshape(1)))


def grad_accumulate(acc, g, mode, scale):
    """the admissible f32 results of one accumulate over whole buffers: (two roundings, one rounding), as f32 tensors.  mode 0 INIT acc = s g,
    1 ADD acc += s g, 2 FOLD g = s g + acc.  The product s g is exact in f64, so the fused form is (f64 sum) -> f32 (a double rounding
    can differ from a true fma only on an exact f64 tie, 2^-29 per element)"""
    s = f32r(scale)
    prod = g.double() * s
    two = prod.float() if mode == 0 else prod.float() + acc.float()
    one = prod.float() if mode == 0 else (prod + acc.double()).float()
    return two, one


# ===================================================================================================================== inputs and cases
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def away(shape, g, lo=0.25):
    """random values with |x| >= lo (terms bounded away from zero)"""
    r = torch.randn(shape, generator=g)
    return torch.where(r >= 0, 1.0, -1.0) * (lo + r.abs())


def _hc(B, N, d, K, dtype='f32', family='normal'):
    return dict(B=B, N=N, d=d, K=K, dtype=dtype, family=family)


D_LIST = [1, 63, 64, 65, 96, 255, 256, 257, 768, 1024, 8192]
K_LIST = [1, 3, 4, 5, 71, 130]
B_LIST = [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16, 17, 255, 256, 257, 512]

# head forward AND backward (the backward of a case runs on the forward reference's xhat / rstd, rounded to f32)
HEAD_CASES = ([_hc(9, 7, d, 71) for d in D_LIST] + [_hc(9, 1, d, 71, 'bf16') for d in (1, 65, 257, 768, 8192)]
              + [_hc(9, 7, 96, K) for K in K_LIST if K != 71] + [_hc(9, 1, 96, 130, 'bf16'), _hc(9, 251, 96, 5), _hc(9, 251, 255, 3, 'bf16')]
              + [_hc(512, 251, 768, 71, 'bf16'), _hc(64, 251, 1024, 71, 'bf16'), _hc(64, 1, 1024, 71)]
              + [_hc(9, 7, 64, 5, 'f32', 'mean100'), _hc(9, 1, 256, 71, 'f32', 'mean100'), _hc(9, 7, 256, 5, 'f32', 'mean100')])
# head backward only: every residue of B against the paired / remainder loop of the T stage, and its b += 256 bias loop
HEAD_BWD_B_CASES = [_hc(B, 1 if B % 2 else 3, 96, 5, 'bf16' if B in (3, 8, 257) else 'f32') for B in B_LIST]
# exact-integer family of the backward: (B, N, d, K, dtype); dX is exact where d is a power of two
HEAD_EXACT_CASES = [(9, 7, 64, 5, 'f32'), (13, 1, 256, 71, 'f32'), (257, 2, 96, 5, 'f32'), (512, 1, 1024, 4, 'bf16'), (17, 3, 257, 130, 'f32'),
                    (4, 1, 1, 1, 'f32'), (8, 2, 8192, 3, 'f32')]


def head_id(c):
    return f"B{c['B']}-N{c['N']}-d{c['d']}-K{c['K']}-{c['dtype']}" + ('' if c['family'] == 'normal' else '-' + c['family'])


def head_inputs(c):
    """x_cls [B,d] (bf16-representable for a bf16 case), gamma, beta, W, bias, dl [B,K]; |gamma|, |W| >= 0.25"""
    B, d, K = c['B'], c['d'], c['K']
    g = _gen(1000 + 7 * B + 13 * d + 31 * K + (1 if c['dtype'] == 'bf16' else 0))
    if c['family'] == 'mean100':
        # rows of mean 100 and standard deviation 0.1 on a 2^-8 grid with d a power of two <= 256: the f32 sum, and so the mean and the
        # centred row, are exact, and the case stays well conditioned in the units above; E[x^2] - mu^2 in f32 loses the variance entirely
        assert d & (d - 1) == 0 and d <= 256
        x = 100.0 + torch.round(0.1 * torch.randn(B, d, generator=g) * 256) / 256
    else:
        x = torch.randn(B, d, generator=g) * 1.5 + 0.3
    if c['dtype'] == 'bf16':
        x = x.to(BF16).float()
    gamma, beta = away((d,), g), torch.randn(d, generator=g)
    W, bias = away((K, d), g), torch.randn(K, generator=g)
    dl = torch.randn(B, K, generator=g) * 0.1
    return dict(x=x, gamma=gamma, beta=beta, W=W, bias=bias, dl=dl)


def head_bwd_inputs(c):
    """the backward's inputs: the f64 forward reference's xhat and rstd rounded to f32 (what a correct forward leaves behind)"""
    i = head_inputs(c)
    out, _ = head_fwd(i['x'], i['gamma'], i['beta'], i['W'], i['bias'])
    i['xhat'], i['rstd'] = out['xhat'].float(), out['rstd'].float()
    return i


def head_exact_inputs(B, d, K):
    g = _gen(5000 + B + 3 * d + 7 * K)
    ri = lambda *s: torch.randint(-2, 3, s, generator=g).float()
    rstd = 2.0 ** torch.randint(-1, 3, (B,), generator=g).float()
    return dict(dl=ri(B, K), xhat=ri(B, d), rstd=rstd, gamma=ri(d), beta=ri(d), W=ri(K, d))


# ---- BCE
BCE_SPECIALS = [0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]
BCE_COUNTS = [1, 1023, 1024, 1025, 71 * 512, 71 * 4096]
# forward: (count, labels, weight, loss_mean)
BCE_FWD_CASES = [(1, 'hard', False, True), (1023, 'soft', True, True), (1024, 'hard', True, False), (1025, 'hard', False, True),
                 (71 * 512, 'hard', True, True), (71 * 512, 'soft', False, False), (71 * 4096, 'soft', True, True), (71 * 4096, 'hard', False, True)]
# backward: (count, labels, weight, upstream form, gscale)
BCE_BWD_CASES = [(1, 'hard', False, 'none', 1.0), (1023, 'soft', True, 'gelem', 2.0 ** -10), (1024, 'hard', True, 'gscalar', 1.0 / 1024),
                 (1025, 'hard', False, 'none', 2.0 ** -10), (71 * 512, 'hard', True, 'gscalar', 1.0 / (71 * 512)), (71 * 512, 'soft', False, 'gelem', 1.0),
                 (71 * 4096, 'soft', True, 'none', 1.0 / (71 * 4096)), (71 * 4096, 'hard', False, 'gelem', 1.0 / (71 * 4096)),
                 (1025, 'soft', True, 'gscalar', 1.0)]


def bce_inputs(count, labels, weight):
    """logits: N(0, 3^2) with every special value at both hard labels (and the soft one) spread over the buffer; the last element is 20 at
    label 0 so the sum's last term is not negligible"""
    g = _gen(2000 + count + (1 if labels == 'soft' else 0) + (2 if weight else 0))
    z = torch.randn(count, generator=g) * 3
    y = (torch.rand(count, generator=g) < 0.3).float()
    if labels == 'soft':
        y = torch.where(torch.rand(count, generator=g) < 0.5, torch.full_like(y, 0.3), y)
    sp = [(s, lab) for s in BCE_SPECIALS for lab in ((0.0, 1.0, 0.3) if labels == 'soft' else (0.0, 1.0))]
    if count >= len(sp):
        stride = count // len(sp)
        for j, (s, lab) in enumerate(sp):
            z[j * stride], y[j * stride] = s, lab
    else:
        for j in range(count):
            z[j], y[j] = sp[(5 * j + 3) % len(sp)]
    if count > 100:
        z[-1], y[-1] = 20.0, 0.0
    w = (0.5 + 2.5 * torch.rand(count, generator=g)) if weight else None
    gelem = away((count,), g) * 0.5
    gscalar = torch.tensor([1.75])
    return dict(z=z, y=y, w=w, gelem=gelem, gscalar=gscalar)


# ---- norm
SUMSQ_COUNTS = [1, 2, 3, 4, 5, 7, 1023, 1024, 100003, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 4, 3 * 2 ** 20 + 5]


def decades(n, g, lo=-6.0, hi=6.0):
    """signed values whose magnitudes are log-uniform over 10^lo .. 10^hi; the LAST element has the largest magnitude, 10^hi"""
    x = 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=g, dtype=F64))
    x = (x * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).float()
    x[-1] = -(10.0 ** hi)
    return x


def sumsq_inputs(count, family):
    g = _gen(3000 + count)
    if family == 'ints':     # values in {-2..2}: the sum stays below 2^24 (4 * (3 * 2^20 + 5) < 2^24) and is an exact integer in any order
        return torch.randint(-2, 3, (count,), generator=g).float()
    return decades(count, g)


# span tables: (offset, count, step offset).  SMALL: every off % 4, counts 1..5, adjacent spans.  BIG: an unaligned head span, an aligned span
# long enough for a second grid-stride trip of both span kernels (1024 * 256 vectors, 4096 * 256 elements), an adjacent unaligned span
SPANS_SMALL = [(0, 1, 0), (5, 2, -1), (10, 3, 0), (15, 4, -2), (21, 5, 0), (26, 5, -1), (32, 4, 0), (39, 3, -2)]
SPANS_BIG = [(3, 1027, -1), (1032, 2 ** 20 + 2 ** 18 + 5, 0), (1032 + 2 ** 20 + 2 ** 18 + 5, 1300, -2), (2 ** 20 + 2 ** 18 + 4002, 1026, 0)]
SPAN_TABLES = dict(small=(SPANS_SMALL, 48), big=(SPANS_BIG, 2 ** 20 + 2 ** 18 + 5100))   # name -> (table, buffer length)


# ---- update
def _ac(count, step, gs, max_norm, decoupled, wd, plow, lr=1e-2):
    return dict(count=count, step=step, gs=gs, max_norm=max_norm, decoupled=decoupled, wd=wd, plow=plow, lr=lr)


ADAMW_CASES = [
    _ac(1, 1, 1.0, 1.0, True, 0.1, True), _ac(255, 2, 0.25, 1e-3, True, 0.1, False), _ac(256, 10, 2.0 ** -10, 0.0, False, 0.1, True),
    _ac(257, 1000, -1.0, -1.0, True, 0.0, False), _ac(2 ** 20, 100000, 1.0, 1.0, True, 0.1, True), _ac(2 ** 20 + 1, 1, 0.25, 1e-3, False, 0.1, True),
    _ac(2 ** 21 + 3, 10, -1.0, 1.0, True, 0.01, True), _ac(257, 100000, 2.0 ** -10, 1.0, False, 0.1, False), _ac(255, 2, 1.0, 1.0, True, 0.0, True),
    _ac(256, 1000, 0.25, 0.0, False, 0.0, False, lr=1e-3), _ac(1, 10, -1.0, 1e-3, False, 0.1, False),
]
# span update: (table name, step, grad_scale, max_norm, decoupled, wd)
ADAMW_SPAN_CASES = [('small', 3, 1.0, 1.0, True, 0.1), ('small', 1000, -1.0, 0.0, False, 0.1), ('big', 3, 0.25, 1e-3, True, 0.1), ('big', 12, 1.0, -1.0, False, 0.0)]
CLIP_CASES = [(1, 1.0), (255, 1e-3), (257, 0.0), (2 ** 20 + 1, 1.0), (2 ** 20 + 1, -1.0), (2 ** 21 + 3, 1e-3)]   # (count, max_norm)


def adamw_id(c):
    return f"n{c['count']}-step{c['step']}-gs{c['gs']:g}-mn{c['max_norm']:g}-{'adamw' if c['decoupled'] else 'adam'}-wd{c['wd']:g}" + ('-plow' if c['plow'] else '')


def adamw_inputs(count, seed=0):
    """p with exact zeros and small entries (the update is then the whole result), gradients spanning 1e-12 .. 1 (eps dominates below 1e-9) with
    one large gradient last so the clip binds, and a state at each gradient's own scale"""
    g = _gen(4000 + count + seed)
    p = torch.randn(count, generator=g)
    r = torch.rand(count, generator=g)
    p = torch.where(r < 0.125, torch.zeros_like(p), torch.where(r < 0.25, p * 1e-3, p))
    gr = decades(count, g, -12.0, 0.0)
    if count > 1:
        gr[-1] = 3.0
    if count > 2:
        gr[0], p[0] = 1e-10, 0.0
    m = gr * (2 * torch.rand(count, generator=g) - 1)
    v = (gr * (0.5 + 1.5 * torch.rand(count, generator=g))) ** 2
    if count == 1:
        p[0], gr[0], m[0], v[0] = 0.03, -3e-10, 1e-10, 4e-20
    return dict(p=p, g=gr, m=m, v=v)


ADAMW_PERTURB = ('eps_inside', 'bias_step_minus_1', 'coupled_for_decoupled', 'no_clip')


def adamw_perturb_applies(name, c, coef):
    """a perturbed reference is asked to lie >= 2 C away only where it differs from the reference by construction: the bias corrections at
    step - 1 do not exist at step 1 and equal those at step to 1e-40 at step 100 000; the two decays coincide at wd = 0; coef = 1 when the clip
    is off or does not bind"""
    if name == 'bias_step_minus_1':
        return 2 <= c['step'] <= 1000
    if name == 'coupled_for_decoupled':
        return c['wd'] > 0
    if name == 'no_clip':
        return coef < 0.5
    return True
