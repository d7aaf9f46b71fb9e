"""
The kernels of csrc/head_opt.hip through the C ABI, against the float64 restatements of tests/head_opt_ref.py, element by element, in the units
and with the constants that tests/test_head_opt_ref.py calibrates on the CPU.  Every output is a slice of a larger buffer filled with a
sentinel whose guard bands must come back bit-identical; every in-place call is checked for "elements outside are untouched" the same way.
Each figure is printed (`RATIO name value`) before it is asserted.
"""
import pytest
import torch

import head_opt_ref as R
from head_opt_ref import C, F32, F64, BF16, ratio
from hiputil import dev, ptr, check, stream
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.hip import lib

pytestmark = pytest.mark.gpu

PAD = 64            # guard band, elements (keeps the interior 16-B aligned)
SENTINEL = -777.25  # exactly representable in f32 and bf16
EINVAL = 1
_BITS = {F32: torch.int32, BF16: torch.int16, torch.int64: torch.int64, torch.uint8: torch.uint8}


def bits(t):
    return t.view(_BITS[t.dtype])


class Guarded:
    """n elements inside a sentinel-filled device buffer.  init: host tensor copied in; interior: a fill of its own for the n elements"""

    def __init__(self, n=None, dtype=F32, init=None, interior=None):
        n = init.numel() if init is not None else n
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device='cuda')
        self.t = self.buf[PAD:PAD + n]
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))
        elif interior is not None:
            self.t.fill_(interior)
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def bands_ok(self):
        b, a = bits(self.buf), bits(self.before)
        return torch.equal(b[:PAD], a[:PAD]) and torch.equal(b[PAD + self.n:], a[PAD + self.n:])

    def untouched(self):
        return torch.equal(bits(self.buf), bits(self.before))

    def outside_untouched(self, index):
        """every element whose interior index is not in `index` (a host int64 tensor) is bit-identical"""
        keep = torch.ones(self.n + 2 * PAD, dtype=torch.bool, device='cuda')
        keep[index.cuda() + PAD] = False
        return torch.equal(bits(self.buf)[keep], bits(self.before)[keep])

    def cpu(self):
        return self.t.detach().cpu()


def report(name, r, cname=None):
    print(f'RATIO {name} {r:.4g}')
    assert r <= C[cname or name], (name, r, C[cname or name])


def span_table(spans):
    return dev(torch.tensor(spans, dtype=torch.int64).reshape(-1, 3))


def workspace():
    return torch.empty(lib().ecgvit_sumsq_workspace(1), dtype=torch.uint8, device='cuda')


# ===================================================================================================================== head forward
def pitched_x(x, N, dtype):
    """[B*N, d] activations with the CLS rows = x and every other token a value a kernel must never read into its result"""
    B, d = x.shape
    X = torch.full((B, N, d), 3.0, dtype=dtype, device='cuda')
    X[:, 0] = x.to(dtype).cuda()
    return X


@pytest.mark.parametrize('c', R.HEAD_CASES, ids=R.head_id)
def test_head_fwd(c):
    B, N, d, K = c['B'], c['N'], c['d'], c['K']
    dtype = BF16 if c['dtype'] == 'bf16' else F32
    i = R.head_inputs(c)
    X = pitched_x(i['x'], N, dtype)
    gd, bd, Wd, biasd = dev(i['gamma']), dev(i['beta']), dev(i['W']), dev(i['bias'])
    logits, xhat, rstd = Guarded(B * K), Guarded(B * d), Guarded(B)
    check(lib().ecgvit_head_fwd(ptr(X), N, ptr(gd), ptr(bd), ptr(Wd), ptr(biasd), logits.ptr, xhat.ptr, rstd.ptr, B, d, K, R.EPS_LN,
                                hip.code(dtype), stream()), 'head_fwd')
    torch.cuda.synchronize()
    ref, mag = R.head_fwd(i['x'], i['gamma'], i['beta'], i['W'], i['bias'])
    for name, got in (('logits', logits), ('xhat', xhat), ('rstd', rstd)):
        assert got.bands_ok(), name
        report('head_fwd.' + name, ratio(got.cpu(), ref[name], mag[name]))


# ===================================================================================================================== head backward
def run_head_bwd(i, B, N, d, K, dtype):
    dd = {k: dev(i[k]) for k in ('dl', 'xhat', 'rstd', 'gamma', 'beta', 'W')}
    out = dict(dW=Guarded(K * d), dbias=Guarded(K), dgamma=Guarded(d), dbeta=Guarded(d), dX=Guarded(B * N * d, dtype, interior=7.0))
    check(lib().ecgvit_head_bwd(ptr(dd['dl']), ptr(dd['xhat']), ptr(dd['rstd']), ptr(dd['gamma']), ptr(dd['beta']), ptr(dd['W']), out['dW'].ptr,
                                out['dbias'].ptr, out['dgamma'].ptr, out['dbeta'].ptr, out['dX'].ptr, N, B, d, K, hip.code(dtype), stream()), 'head_bwd')
    torch.cuda.synchronize()
    for k, o in out.items():
        assert o.bands_ok(), k
    dX = out['dX'].t.view(B, N, d)
    assert bool((bits(dX[:, 1:]) == 0).all()), 'dX is not exactly +0 off the CLS rows'
    return out, dX[:, 0].cpu()


@pytest.mark.parametrize('c', R.HEAD_CASES + R.HEAD_BWD_B_CASES, ids=R.head_id)
def test_head_bwd(c):
    B, N, d, K = c['B'], c['N'], c['d'], c['K']
    dtype = BF16 if c['dtype'] == 'bf16' else F32
    i = R.head_bwd_inputs(c)
    out, dx_cls = run_head_bwd(i, B, N, d, K, dtype)
    ref, mag = R.head_bwd(i['dl'], i['xhat'], i['rstd'], i['gamma'], i['beta'], i['W'])
    for k in ('dW', 'dbias', 'dgamma', 'dbeta'):
        report('head_bwd.' + k, ratio(out[k].cpu(), ref[k], mag[k]))
    report('head_bwd.dX', ratio(dx_cls, ref['dX'], mag['dX'], dtype == BF16))


@pytest.mark.parametrize('case', R.HEAD_EXACT_CASES, ids=str)
def test_head_bwd_exact_integers(case):
    """small-integer inputs, power-of-two rstd, every sum below 2^24: the four parameter gradients are the integer result bit for bit in any
    summation order, so an off-by-one in any loop bound is an integer difference; with d a power of two dX is exact as well"""
    B, N, d, K, dt = case
    dtype = BF16 if dt == 'bf16' else F32
    i = R.head_exact_inputs(B, d, K)
    out, dx_cls = run_head_bwd(i, B, N, d, K, dtype)
    ref, _ = R.head_bwd(i['dl'], i['xhat'], i['rstd'], i['gamma'], i['beta'], i['W'])
    for k in ('dW', 'dbias', 'dgamma', 'dbeta'):
        assert torch.equal(out[k].cpu().double(), ref[k].reshape(-1)), k
    if d & (d - 1) == 0:
        assert torch.equal(dx_cls.double(), ref['dX'].to(dtype).double()), 'dX'
    print(f'EXACT head_bwd {case}')


# ===================================================================================================================== BCE
@pytest.mark.parametrize('case', R.BCE_FWD_CASES, ids=str)
def test_bce_fwd(case):
    count, labels, weight, mean = case
    i = R.bce_inputs(count, labels, weight)
    zd, yd, wd = dev(i['z']), dev(i['y']), (dev(i['w']) if weight else None)
    ref, mag = R.bce_fwd(i['z'], i['y'], i['w'])
    runs = []
    for _ in range(2):
        le, lm = Guarded(count), Guarded(1)
        check(lib().ecgvit_bce_fwd(ptr(zd), ptr(yd), ptr(wd), le.ptr, lm.ptr if mean else None, count, stream()), 'bce_fwd')
        torch.cuda.synchronize()
        assert le.bands_ok() and (lm.bands_ok() if mean else lm.untouched())
        runs.append((le, lm))
    assert torch.equal(bits(runs[0][0].buf), bits(runs[1][0].buf)) and torch.equal(bits(runs[0][1].buf), bits(runs[1][1].buf)), 'not deterministic'
    report('bce_fwd.loss_elem', ratio(runs[0][0].cpu(), ref['loss_elem'], mag['loss_elem']))
    if mean:
        report('bce_fwd.loss_mean', ratio(runs[0][1].cpu(), ref['loss_mean'], mag['loss_mean']))


def test_bce_fwd_nan_logit():
    i = R.bce_inputs(1025, 'hard', False)
    i['z'][517], i['y'][517] = float('nan'), 0.0
    le, lm = Guarded(1025), Guarded(1)
    check(lib().ecgvit_bce_fwd(ptr(dev(i['z'])), ptr(dev(i['y'])), None, le.ptr, lm.ptr, 1025, stream()), 'bce_fwd')
    torch.cuda.synchronize()
    got = le.cpu()
    assert le.bands_ok() and lm.bands_ok()
    assert bool(torch.isnan(got[517])) and int(torch.isnan(got).sum()) == 1 and bool(torch.isnan(lm.cpu()).all())


@pytest.mark.parametrize('case', R.BCE_BWD_CASES, ids=str)
def test_bce_bwd(case):
    count, labels, weight, form, gscale = case
    i = R.bce_inputs(count, labels, weight)
    zd, yd, wd = dev(i['z']), dev(i['y']), (dev(i['w']) if weight else None)
    ge = dev(i['gelem']) if form == 'gelem' else None
    gsc = dev(i['gscalar']) if form == 'gscalar' else None
    dz = Guarded(count)
    check(lib().ecgvit_bce_bwd(ptr(zd), ptr(yd), ptr(wd), ptr(gsc), ptr(ge), gscale, dz.ptr, count, stream()), 'bce_bwd')
    torch.cuda.synchronize()
    assert dz.bands_ok()
    ref, mag = R.bce_bwd(i['z'], i['y'], i['w'], gelem=i['gelem'] if form == 'gelem' else None, gscalar=i['gscalar'] if form == 'gscalar' else None,
                         gscale=gscale)
    report('bce_bwd.dlogits', ratio(dz.cpu(), ref['dlogits'], mag['dlogits']))


# ===================================================================================================================== norm
@pytest.mark.parametrize('count', R.SUMSQ_COUNTS)
def test_sumsq(count):
    ws = workspace()
    for family in ('decades', 'ints'):
        g = R.sumsq_inputs(count, family)
        gd = Guarded(init=g)       # the gradient is an input: it must come back untouched, and nothing past its end may be read into the sum
        out = Guarded(1)
        check(lib().ecgvit_sumsq(gd.ptr, count, out.ptr, ptr(ws), stream()), 'sumsq')
        torch.cuda.synchronize()
        assert out.bands_ok() and gd.untouched()
        ref, mag = R.sumsq(g)
        if family == 'ints':
            assert float(out.cpu()) == float(ref['out']), (float(out.cpu()), float(ref['out']))
            print(f'EXACT sumsq {count}')
        else:
            report('sumsq.out', ratio(out.cpu(), ref['out'], mag['out']))


@pytest.mark.parametrize('name', list(R.SPAN_TABLES))
def test_sumsq_spans(name):
    spans, n = R.SPAN_TABLES[name]
    ws, tab, total = workspace(), span_table(spans), sum(s[1] for s in spans)
    for family in ('decades', 'ints'):
        g = R.sumsq_inputs(n, family)
        if family == 'decades':
            g[spans[-1][0] + spans[-1][1] - 1], g[-1] = g[-1].clone(), 1.0
        else:
            outside = torch.ones(n, dtype=torch.bool)
            outside[R.span_index(spans)] = False
            g[outside] = 1000.0      # an element read from outside the spans shows
        gd, out = Guarded(init=g), Guarded(1)
        check(lib().ecgvit_sumsq_spans(gd.ptr, ptr(tab), len(spans), total, out.ptr, ptr(ws), stream()), 'sumsq_spans')
        torch.cuda.synchronize()
        assert out.bands_ok() and gd.untouched()
        ref, mag = R.sumsq_spans(g, spans)
        if family == 'ints':
            assert float(out.cpu()) == float(ref['out']), (float(out.cpu()), float(ref['out']))
            print(f'EXACT sumsq_spans {name}')
        else:
            report('sumsq_spans.out', ratio(out.cpu(), ref['out'], mag['out']))


# ===================================================================================================================== update
HYPER = dict(b1=0.9, b2=0.999, eps=1e-8)


def device_sumsq(gd, count):
    ss = Guarded(1)
    check(lib().ecgvit_sumsq(gd.data_ptr(), count, ss.ptr, ptr(workspace()), stream()), 'sumsq')
    torch.cuda.synchronize()
    assert ss.bands_ok()
    ss.before = ss.buf.clone()      # from here on an input: later calls must leave it alone
    return ss


@pytest.mark.parametrize('c', R.ADAMW_CASES, ids=R.adamw_id)
def test_adamw_step(c):
    """two consecutive steps; each is held to the fp64 restatement fed the kernel's own f32 state (one-step error)"""
    n = c['count']
    i = R.adamw_inputs(n)
    p, m, v = Guarded(init=i['p']), Guarded(init=i['m']), Guarded(init=i['v'])
    gd = Guarded(init=i['g'])
    plow = Guarded(n, BF16) if c['plow'] else None
    no = Guarded(2)
    ss = device_sumsq(gd.t, n)
    ssh = ss.cpu()
    for step in (c['step'], c['step'] + 1):
        state = [t.cpu() for t in (p, m, v)]
        check(lib().ecgvit_adamw_step(p.ptr, gd.ptr, m.ptr, v.ptr, plow.ptr if plow else None, n, ss.ptr, c['gs'], c['max_norm'], c['lr'], HYPER['b1'],
                                      HYPER['b2'], HYPER['eps'], c['wd'], step, int(c['decoupled']), no.ptr, stream()), 'adamw')
        torch.cuda.synchronize()
        assert p.bands_ok() and m.bands_ok() and v.bands_ok() and no.bands_ok() and gd.untouched() and ss.untouched()
        ref, mag = R.adamw(state[0], i['g'], state[1], state[2], ssh, c['gs'], c['max_norm'], c['lr'], wd=c['wd'], step=step, decoupled=c['decoupled'], **HYPER)
        for k, got in (('p', p), ('m', m), ('v', v)):
            report('adamw.' + k, ratio(got.cpu(), ref[k], mag[k]))
        report('adamw.norm', ratio(no.cpu()[:1], ref['norm'], mag['norm']))
        assert float(no.cpu()[1]) == 1.0
        if plow:
            assert plow.bands_ok() and torch.equal(bits(plow.t), bits(p.t.to(BF16))), 'p_lowp != p.to(bfloat16)'


def test_adamw_trajectory_against_torch_optim():
    """20 steps against clip_grad_norm_ + torch.optim.AdamW in fp64: the accumulated error of 20 one-step errors (each <= C['adamw.p'] u mag)"""
    n = 1027
    i = R.adamw_inputs(n)
    pt = torch.nn.Parameter(i['p'].double().clone())
    lr, b1, b2, eps, wd = (R.f32r(s) for s in (1e-2, 0.9, 0.999, 1e-8, 0.1))
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v, no = Guarded(init=i['p']), Guarded(init=torch.zeros(n)), Guarded(init=torch.zeros(n)), Guarded(2)
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for step in range(1, 21):
        gr = R.decades(n, g, -12.0, 0.0) * (3.0 if step % 2 else 0.1)
        pt.grad = gr.double().clone()
        torch.nn.utils.clip_grad_norm_([pt], 1.0, error_if_nonfinite=True)
        opt.step()
        gd = dev(gr)
        ss = device_sumsq(gd, n)
        check(lib().ecgvit_adamw_step(p.ptr, ptr(gd), m.ptr, v.ptr, None, n, ss.ptr, 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, step, 1, no.ptr, stream()), 'adamw')
        torch.cuda.synchronize()
        # unit: |p| + the step's size (|update| <= lr / bc1 * |m| / denom <= ~lr whatever cancels inside it)
        worst = max(worst, ratio(p.cpu(), pt.detach(), pt.detach().abs() + lr))
    print(f'RATIO adamw.trajectory20 {worst:.4g}')
    assert worst <= 20 * C['adamw.p'] and p.bands_ok() and m.bands_ok() and v.bands_ok()


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_adamw_nonfinite_gradient_updates_nothing(bad):
    n = 1025
    i = R.adamw_inputs(n)
    i['g'][3] = bad
    spans = [(1, 6, 0), (16, 1000, -1)]
    for use_spans in (False, True):
        p, m, v, plow, no = Guarded(init=i['p']), Guarded(init=i['m']), Guarded(init=i['v']), Guarded(n, BF16), Guarded(2)
        gd = dev(i['g'])
        ss = device_sumsq(gd, n)
        if use_spans:
            check(lib().ecgvit_adamw_step_spans(p.ptr, ptr(gd), m.ptr, v.ptr, plow.ptr, ptr(span_table(spans)), 2, 1006, ss.ptr, 1.0, 1.0, 1e-2, 0.9, 0.999,
                                                1e-8, 0.1, 5, 1, no.ptr, stream()), 'adamw_spans')
        else:
            check(lib().ecgvit_adamw_step(p.ptr, ptr(gd), m.ptr, v.ptr, plow.ptr, n, ss.ptr, 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 5, 1, no.ptr, stream()), 'adamw')
        torch.cuda.synchronize()
        assert p.untouched() and m.untouched() and v.untouched() and plow.untouched()
        assert float(no.cpu()[1]) == 0.0 and no.bands_ok()


@pytest.mark.parametrize('case', R.ADAMW_SPAN_CASES, ids=str)
def test_adamw_step_spans(case):
    """each span against the fp64 reference at its own step (not against the whole-buffer kernel); outside the spans nothing changes"""
    name, step, gs, max_norm, decoupled, wd = case
    spans, n = R.SPAN_TABLES[name]
    total, idx = sum(s[1] for s in spans), R.span_index(spans)
    i = R.adamw_inputs(n, seed=11)
    p, m, v, plow, no = Guarded(init=i['p']), Guarded(init=i['m']), Guarded(init=i['v']), Guarded(n, BF16), Guarded(2)
    gd, tab = Guarded(init=i['g']), span_table(spans)
    ss = Guarded(1)
    check(lib().ecgvit_sumsq_spans(gd.ptr, ptr(tab), len(spans), total, ss.ptr, ptr(workspace()), stream()), 'sumsq_spans')
    check(lib().ecgvit_adamw_step_spans(p.ptr, gd.ptr, m.ptr, v.ptr, plow.ptr, ptr(tab), len(spans), total, ss.ptr, gs, max_norm, 1e-2, HYPER['b1'], HYPER['b2'],
                                        HYPER['eps'], wd, step, int(decoupled), no.ptr, stream()), 'adamw_spans')
    torch.cuda.synchronize()
    ref, mag = R.adamw_spans(i['p'], i['g'], i['m'], i['v'], spans, ss.cpu(), step=step, grad_scale=gs, max_norm=max_norm, decoupled=decoupled, wd=wd)
    for k, got in (('p', p), ('m', m), ('v', v), ('p_lowp', plow)):
        assert got.outside_untouched(idx), f'{k} changed outside the spans'
    assert gd.untouched() and no.bands_ok()
    for k, got in (('p', p), ('m', m), ('v', v)):
        report('adamw_spans.' + k, ratio(got.cpu()[idx], ref[k][idx], mag[k][idx]), 'adamw.' + k)
    report('adamw_spans.norm', ratio(no.cpu()[:1], ref['norm'], mag['norm']), 'adamw.norm')
    assert float(no.cpu()[1]) == 1.0
    assert torch.equal(bits(plow.t[idx.cuda()]), bits(p.t[idx.cuda()].to(BF16))), 'p_lowp != p.to(bfloat16) inside the spans'


@pytest.mark.parametrize('case', R.CLIP_CASES, ids=str)
def test_clip_scale(case):
    count, max_norm = case
    i = R.adamw_inputs(count, seed=5)
    gd, no = Guarded(init=i['g']), Guarded(2)
    ss = device_sumsq(gd.t, count)
    check(lib().ecgvit_clip_scale(gd.ptr, count, ss.ptr, max_norm, no.ptr, stream()), 'clip_scale')
    torch.cuda.synchronize()
    assert gd.bands_ok() and no.bands_ok() and ss.untouched()
    ref, mag = R.clip_scale(i['g'], ss.cpu(), max_norm)
    report('clip_scale.g', ratio(gd.cpu(), ref['g'], mag['g']))
    report('clip_scale.norm', ratio(no.cpu()[:1], ref['norm'], mag['norm']))
    if max_norm <= 0:
        assert gd.untouched(), 'max_norm <= 0 must leave every bit alone'


def test_clip_scale_nonfinite_norm_leaves_every_bit():
    i = R.adamw_inputs(1025, seed=5)
    gd, no = Guarded(init=i['g']), Guarded(2)
    ss = Guarded(init=torch.tensor([float('inf')]))
    check(lib().ecgvit_clip_scale(gd.ptr, 1025, ss.ptr, 1.0, no.ptr, stream()), 'clip_scale')
    torch.cuda.synchronize()
    assert gd.untouched() and float(no.cpu()[1]) == 0.0 and no.bands_ok()


# ===================================================================================================================== accumulate
ACC_TABLES = dict(small=(R.SPANS_SMALL, 48), tails=([(0, 1027, 0), (1029, 514, 0), (1544, 4099, 0), (5646, 7, 0)], 5700))


@pytest.mark.parametrize('name', list(ACC_TABLES))
@pytest.mark.parametrize('mode', [hip.ACC_INIT, hip.ACC_ADD, hip.ACC_FOLD])
@pytest.mark.parametrize('scale', [1.0, 0.3])
def test_grad_accumulate(name, mode, scale):
    spans, n = ACC_TABLES[name]
    total, idx = sum(s[1] for s in spans), R.span_index(spans)
    g = torch.Generator().manual_seed(77 + mode)
    a0, g0 = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    acc, gr = Guarded(init=a0), Guarded(init=g0)
    check(lib().ecgvit_grad_accumulate(acc.ptr, gr.ptr, ptr(span_table(spans)), len(spans), total, mode, scale, stream()), 'grad_accumulate')
    torch.cuda.synchronize()
    written, other = (gr, acc) if mode == hip.ACC_FOLD else (acc, gr)
    assert other.untouched() and written.outside_untouched(idx)
    two, one = R.grad_accumulate(a0, g0, mode, scale)
    got = written.cpu()[idx]
    if scale == 1.0:
        assert torch.equal(two, one) and torch.equal(bits(got), bits(two[idx])), 'scale = 1 must be bit-exact'
    else:   # the compiler may contract scale * g + acc into one fused multiply-add: either rounding, element by element
        assert bool(((bits(got) == bits(two[idx])) | (bits(got) == bits(one[idx]))).all())


# ===================================================================================================================== transpose
# (rows, cols, element offset): every matrix of the table, with gaps between them; the sixth sits at an offset with off % 8 != 0
TR_MATS = [(1, 1, 0), (63, 65, 8), (64, 64, 4112), (72, 136, 8216), (768, 2304, 18016), (64, 64, 1787493), (130, 70, 1791600)]
TR_LEN = 1791600 + 130 * 70 + 20


@pytest.mark.parametrize('pick', [(4,), (1, 5), (0, 1, 2, 3, 4, 5, 6)], ids=['nmat1', 'nmat2', 'nmat7'])
def test_transpose_bf16_batched(pick):
    g = torch.Generator().manual_seed(9)
    src_h = torch.randn(TR_LEN, generator=g).to(BF16)
    src, dst = Guarded(init=src_h, dtype=BF16), Guarded(TR_LEN, BF16)
    table, tiles, inside = [], 0, []
    for j in pick:
        r, c, off = TR_MATS[j]
        table.append([off, r, c, tiles])
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
        inside.append(torch.arange(off, off + r * c))
    check(lib().ecgvit_transpose_bf16_batched(src.ptr, dst.ptr, ptr(dev(torch.tensor(table, dtype=torch.int64))), len(table), tiles, stream()), 'transpose')
    torch.cuda.synchronize()
    assert src.untouched() and dst.outside_untouched(torch.cat(inside)), 'a gap between the matrices was written'
    got = dst.cpu()
    for j in pick:
        r, c, off = TR_MATS[j]
        assert torch.equal(got[off:off + r * c].view(c, r), src_h[off:off + r * c].view(r, c).T), TR_MATS[j]


# ===================================================================================================================== casts
def _same_or_both_nan(got, want):
    nan = torch.isnan(want.float())
    return bool(torch.isnan(got.float())[nan].all()) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def test_cast_f32_to_bf16_edges():
    """every tie (low half 0x8000) and its two neighbours over all 65536 high halves: +-0, denormals, +-inf, NaN, and 0x7f7f8000.., the largest
    f32 values, which round to bf16 inf; random bit patterns fill up to 2^20 + 1"""
    n = 2 ** 20 + 1
    hi = torch.arange(65536, dtype=torch.int64) << 16
    pat = torch.cat([hi | 0x8000, hi | 0x7fff, hi | 0x8001, hi])
    g = torch.Generator().manual_seed(4)
    pat = torch.cat([pat, torch.randint(0, 2 ** 32, (n - pat.numel(),), generator=g)])
    x = torch.where(pat >= 2 ** 31, pat - 2 ** 32, pat).to(torch.int32).view(F32)
    out = Guarded(n, BF16)
    check(lib().ecgvit_cast_f32_to_bf16(ptr(dev(x)), out.ptr, n, stream()), 'cast')
    torch.cuda.synchronize()
    assert out.bands_ok() and _same_or_both_nan(out.cpu(), x.to(BF16))
    assert bool(torch.isinf(out.cpu()[(0x7f7f)].float())), '0x7f7f8000 rounds to inf'


def test_cast_bf16_to_f32_edges():
    n = 2 ** 20 + 1
    pat = (torch.arange(n, dtype=torch.int64) * 40503) % 65536      # every bf16 pattern, 16 times over
    b = torch.where(pat >= 2 ** 15, pat - 2 ** 16, pat).to(torch.int16).view(BF16)
    out = Guarded(n)
    check(lib().ecgvit_cast_bf16_to_f32(ptr(dev(b)), out.ptr, n, stream()), 'cast')
    torch.cuda.synchronize()
    want = (pat << 16)
    want = torch.where(want >= 2 ** 31, want - 2 ** 32, want).to(torch.int32).view(F32)
    assert out.bands_ok() and _same_or_both_nan(out.cpu(), want)


# ===================================================================================================================== refusals
def test_host_side_refusals_leave_outputs_untouched():
    """only what the launchers decide before any launch; every pointer passed is valid for the sizes a launch would use"""
    L = lib()
    s = stream()
    a, b, c, e = (dev(torch.ones(64)) for _ in range(4))
    outs = [Guarded(64) for _ in range(5)]
    lowp = Guarded(64, BF16)
    o = [x.ptr for x in outs]
    ws = workspace()
    tab = span_table([(0, 4, 0)])
    big = 8193
    calls = {
        'bce_fwd count 0': L.ecgvit_bce_fwd(ptr(a), ptr(b), None, o[0], o[1], 0, s),
        'bce_bwd count 0': L.ecgvit_bce_bwd(ptr(a), ptr(b), None, None, None, 1.0, o[0], 0, s),
        'head_fwd d 8193': L.ecgvit_head_fwd(ptr(a), 1, ptr(b), ptr(c), ptr(e), ptr(e), o[0], o[1], o[2], 1, big, 1, 1e-5, hip.F32, s),
        'head_bwd d 8193': L.ecgvit_head_bwd(ptr(a), ptr(b), ptr(c), ptr(e), ptr(e), ptr(e), o[0], o[1], o[2], o[3], o[4], 1, 1, big, 1, hip.F32, s),
        'sumsq count 0': L.ecgvit_sumsq(ptr(a), 0, o[0], ptr(ws), s),
        'sumsq count -1': L.ecgvit_sumsq(ptr(a), -1, o[0], ptr(ws), s),
        'sumsq misaligned': L.ecgvit_sumsq(ptr(a) + 4, 8, o[0], ptr(ws), s),
        'adamw count 0': L.ecgvit_adamw_step(o[0], ptr(a), o[1], o[2], lowp.ptr, 0, ptr(b), 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 1, 1, o[3], s),
        'adamw step 0': L.ecgvit_adamw_step(o[0], ptr(a), o[1], o[2], lowp.ptr, 64, ptr(b), 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 0, 1, o[3], s),
        'adamw NULL sumsq': L.ecgvit_adamw_step(o[0], ptr(a), o[1], o[2], lowp.ptr, 64, None, 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1, 1, 1, o[3], s),
        'adamw_spans NULL sumsq': L.ecgvit_adamw_step_spans(o[0], ptr(a), o[1], o[2], lowp.ptr, ptr(tab), 1, 4, None, 1.0, 1.0, 1e-2, 0.9, 0.999, 1e-8, 0.1,
                                                            1, 1, o[3], s),
        'clip_scale count 0': L.ecgvit_clip_scale(o[0], 0, ptr(b), 1.0, o[3], s),
        'clip_scale NULL sumsq': L.ecgvit_clip_scale(o[0], 64, None, 1.0, o[3], s),
        'accumulate mode 3': L.ecgvit_grad_accumulate(o[0], o[1], ptr(tab), 1, 4, 3, 1.0, s),
        'cast count 0': L.ecgvit_cast_f32_to_bf16(ptr(a), lowp.ptr, 0, s),
        'cast back count 0': L.ecgvit_cast_bf16_to_f32(lowp.ptr, o[0], 0, s),
    }
    torch.cuda.synchronize()
    for what, rc in calls.items():
        assert rc == EINVAL, (what, rc)
    assert all(x.untouched() for x in outs) and lowp.untouched()
