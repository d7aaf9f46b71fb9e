"""
CPU tests that pin tests/head_opt_ref.py: the float64 restatements agree with torch itself (autograd through layer_norm + linear +
binary_cross_entropy_with_logits; clip_grad_norm_ + torch.optim.AdamW / Adam), and every committed constant C[name] sits >= 4x above the plain
f32 restatement and <= 1/2 x below every applicable perturbed reference, for every case tests/test_gpu_head_opt.py runs.
"""
import pytest
import torch

import head_opt_ref as R
from head_opt_ref import C, F32, F64, BF16, ratio


def _close(a, b, what, tol=1e-12, scale=None):
    """max |a - b| <= tol * max |b| (or * scale: the largest magnitude of the terms, where the result itself cancels to nothing)"""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    err, scale = float((a - b).abs().max()), float(b.abs().max()) if scale is None else scale
    assert err <= tol * max(scale, 1e-300), (what, err, scale)


# ===================================================================================================================== f64 against torch
def _torch_head(i):
    x = i['x'].double().requires_grad_(True)
    pr = [i[k].double().requires_grad_(True) for k in ('gamma', 'beta', 'W', 'bias')]
    z = torch.nn.functional.linear(torch.nn.functional.layer_norm(x, (x.shape[1],), pr[0], pr[1], R.f32r(R.EPS_LN)), pr[2], pr[3])
    return x, pr, z


@pytest.mark.parametrize('c', R.HEAD_CASES + R.HEAD_BWD_B_CASES, ids=R.head_id)
def test_f64_head_and_bce_agree_with_torch(c):
    i = R.head_inputs(c)
    B, K = c['B'], c['K']
    g = torch.Generator().manual_seed(7)
    y = torch.where(torch.rand(B, K, generator=g) < 0.5, torch.full((B, K), 0.3), (torch.rand(B, K, generator=g) < 0.3).float())
    w = 0.5 + torch.rand(B, K, generator=g)
    x, pr, z = _torch_head(i)
    out, _ = R.head_fwd(i['x'], i['gamma'], i['beta'], i['W'], i['bias'])
    _close(out['logits'], z.detach(), 'logits')
    le = torch.nn.functional.binary_cross_entropy_with_logits(z, y.double(), weight=w.double(), reduction='none')
    lo, _ = R.bce_fwd(out['logits'].reshape(-1), y.reshape(-1), w.reshape(-1))
    _close(lo['loss_elem'], le.detach(), 'loss_elem')
    _close(lo['loss_mean'], le.mean().detach(), 'loss_mean')
    le.mean().backward()
    dl, _ = R.bce_bwd(out['logits'].reshape(-1), y.reshape(-1), w.reshape(-1), gscale=1.0)
    dl = dl['dlogits'].reshape(B, K) / (B * K)
    bo, bm = R.head_bwd(dl, out['xhat'], out['rstd'], i['gamma'], i['beta'], i['W'])
    for name, ref in (('dgamma', pr[0].grad), ('dbeta', pr[1].grad), ('dW', pr[2].grad), ('dbias', pr[3].grad), ('dX', x.grad)):
        # d = 1: xhat, dgamma and dX are identically zero; the scale is that of the gradient's terms, sum |dl| |W|
        _close(bo[name], ref, name, scale=float(bm['dbeta'].max()) if c['d'] == 1 else None)


def test_f64_bce_agrees_with_torch_on_saturated_logits():
    for count, labels, weight, _ in R.BCE_FWD_CASES:
        i = R.bce_inputs(count, labels, weight)
        z = i['z'].double().requires_grad_(True)
        le = torch.nn.functional.binary_cross_entropy_with_logits(z, i['y'].double(), weight=None if i['w'] is None else i['w'].double(), reduction='none')
        out, mag = R.bce_fwd(i['z'], i['y'], i['w'])
        # torch forms (1 - y) z - log_sigmoid(z) and so carries |z| through a cancellation even at y = 0 (z = -88: it returns 0, the loss is
        # 6e-39): its own terms are part of the unit here.  1e-6 u = 6e-14 of them
        wz = i['z'].double().abs() * (1.0 if i['w'] is None else i['w'].double())
        assert ratio(out['loss_elem'], le.detach(), mag['loss_elem'] + wz) < 1e-6
        _close(out['loss_mean'], le.mean().detach(), 'loss_mean')
        (le * i['gelem'].double()).sum().backward()
        bo, bm = R.bce_bwd(i['z'], i['y'], i['w'], gelem=i['gelem'])
        assert ratio(bo['dlogits'], z.grad, bm['dlogits']) < 1e-6


@pytest.mark.parametrize('decoupled,wd,max_norm,gs', [(True, 0.1, 1.0, 1.0), (False, 0.1, 1e-3, 0.25), (True, 0.0, 1.0, -1.0), (False, 0.0, 1.0, 2.0 ** -10)])
def test_f64_adamw_trajectory_agrees_with_torch(decoupled, wd, max_norm, gs):
    n = 257
    i = R.adamw_inputs(n)
    lr, b1, b2, eps, wd = (R.f32r(s) for s in (1e-2, 0.9, 0.999, 1e-8, wd))
    pt = torch.nn.Parameter(i['p'].double().clone())
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = i['p'].double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    g = torch.Generator().manual_seed(3)
    for step in range(1, 21):
        gr = R.decades(n, g, -12.0, 0.0) * (3.0 if step % 2 else 0.1)
        pt.grad = gr.double() * gs
        tn = torch.nn.utils.clip_grad_norm_([pt], R.f32r(max_norm), error_if_nonfinite=True)
        opt.step()
        ss, _ = R.sumsq(gr)
        out, _ = R.adamw(p, gr, m, v, ss['out'], gs, max_norm, lr, b1, b2, eps, wd, step, decoupled)
        p, m, v = out['p'], out['m'], out['v']
        _close(out['norm'], tn.detach(), 'norm')
        _close(p, pt.detach(), f'p at step {step}')
    st = opt.state[pt]
    _close(m, st['exp_avg'], 'm')
    _close(v, st['exp_avg_sq'], 'v')


def test_f32_adamw_trajectory_stays_within_the_gpu_tests_bound():
    """the 20-step trajectory test_gpu_head_opt.py runs on the kernel, run on the plain f32 restatement: its distance from torch.optim in fp64, in
    units of u (|p| + lr), is <= a quarter of the 20 C['adamw.p'] the GPU test allows (20 one-step errors; |update| <= ~lr per step)"""
    n = 1027
    i = R.adamw_inputs(n)
    lr, b1, b2, eps, wd = (R.f32r(s) for s in (1e-2, 0.9, 0.999, 1e-8, 0.1))
    pt = torch.nn.Parameter(i['p'].double().clone())
    opt = torch.optim.AdamW([pt], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p, m, v = i['p'], torch.zeros(n), torch.zeros(n)
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for step in range(1, 21):
        gr = R.decades(n, g, -12.0, 0.0) * (3.0 if step % 2 else 0.1)
        pt.grad = gr.double().clone()
        torch.nn.utils.clip_grad_norm_([pt], 1.0, error_if_nonfinite=True)
        opt.step()
        out, _ = R.adamw(p, gr, m, v, R.sumsq(gr, dtype=F32)[0]['out'], 1.0, 1.0, lr, b1, b2, eps, wd, step, True, dtype=F32)
        p, m, v = out['p'], out['m'], out['v']
        worst = max(worst, ratio(p, pt.detach(), pt.detach().abs() + lr))
    print(f'CAL adamw.trajectory20 f32 {worst:.3g}')
    assert worst <= 20 * C['adamw.p'] / 4


# ===================================================================================================================== calibration
# Each calibrate_* returns a list of (constant's name, f32 restatement's worst ratio, {perturbation: its worst ratio}).  The tests assert
# f32 <= C / 4 and every perturbation >= 2 C; the table in head_opt_ref.py is the worst / nearest of these over the case lists.
def _cal(name, ref, mag, f32, perturbed, bf16_out=False):
    return name, ratio(f32.to(BF16) if bf16_out else f32, ref, mag, bf16_out), {k: ratio(v, ref, mag) for k, v in perturbed.items()}


def calibrate_head_fwd(c):
    i = R.head_inputs(c)
    a = (i['x'], i['gamma'], i['beta'], i['W'], i['bias'])
    ref, mag = R.head_fwd(*a)
    f32, _ = R.head_fwd(*a, dtype=F32)
    drop, _ = R.head_fwd(*a, perturb='drop_last_term')
    eo, _ = R.head_fwd(*a, perturb='eps_outside')
    rows = [_cal('head_fwd.logits', ref['logits'], mag['logits'], f32['logits'], dict(drop_last_term=drop['logits'])),
            _cal('head_fwd.rstd', ref['rstd'], mag['rstd'], f32['rstd'], dict(eps_outside=eo['rstd']))]
    px = dict(eps_outside=eo['xhat'])
    if c['d'] == 1:
        px = {}      # one column: xhat is identically zero wherever eps sits
    if c['family'] == 'mean100':
        # xhat's unit is 2000 |xhat| here (|x| + |mu| against |x - mu|): a misplaced eps, 4e-4 of xhat, is below it and is held on rstd;
        # what this family is for is the one-pass variance, which must show in both
        op, _ = R.head_fwd(*a, dtype=F32, perturb='one_pass_var')
        rows[1][2]['one_pass_var_f32'] = ratio(op['rstd'], ref['rstd'], mag['rstd'])
        px = dict(one_pass_var_f32=op['xhat'])
    rows.append(_cal('head_fwd.xhat', ref['xhat'], mag['xhat'], f32['xhat'], px))
    return rows


def calibrate_head_bwd(c):
    i = R.head_bwd_inputs(c)
    a = (i['dl'], i['xhat'], i['rstd'], i['gamma'], i['beta'], i['W'])
    ref, mag = R.head_bwd(*a)
    f32, _ = R.head_bwd(*a, dtype=F32)
    row, _ = R.head_bwd(*a, perturb='drop_last_row')
    term, _ = R.head_bwd(*a, perturb='drop_last_term')
    # d = 1: xhat, and with it dgamma, is identically zero
    rows = [_cal('head_bwd.' + k, ref[k], mag[k], f32[k], {} if (k == 'dgamma' and c['d'] == 1) else dict(drop_last_row=row[k]))
            for k in ('dW', 'dbias', 'dgamma', 'dbeta')]
    # d = 1: dX = rstd (g - mean(g) - 0) is identically zero, perturbed or not
    rows.append(_cal('head_bwd.dX', ref['dX'], mag['dX'], f32['dX'], {} if c['d'] == 1 else dict(drop_last_term=term['dX']), c['dtype'] == 'bf16'))
    return rows


def calibrate_bce_fwd(count, labels, weight):
    i = R.bce_inputs(count, labels, weight)
    ref, mag = R.bce_fwd(i['z'], i['y'], i['w'])
    f32, _ = R.bce_fwd(i['z'], i['y'], i['w'], dtype=F32)
    drop, _ = R.bce_fwd(i['z'], i['y'], i['w'], perturb='drop_last_term')
    return [_cal('bce_fwd.loss_elem', ref['loss_elem'], mag['loss_elem'], f32['loss_elem'], dict(drop_last_term=drop['loss_elem'])),
            _cal('bce_fwd.loss_mean', ref['loss_mean'], mag['loss_mean'], f32['loss_mean'], dict(drop_last_term=drop['loss_mean']) if count > 1 else {})]


def bce_bwd_args(i, form, gscale):
    return dict(w=i['w'], gelem=i['gelem'] if form == 'gelem' else None, gscalar=i['gscalar'] if form == 'gscalar' else None, gscale=gscale)


def calibrate_bce_bwd(count, labels, weight, form, gscale):
    i = R.bce_inputs(count, labels, weight)
    kw = bce_bwd_args(i, form, gscale)
    ref, mag = R.bce_bwd(i['z'], i['y'], **kw)
    f32, _ = R.bce_bwd(i['z'], i['y'], dtype=F32, **kw)
    drop, _ = R.bce_bwd(i['z'], i['y'], perturb='drop_last_term', **kw)
    return [_cal('bce_bwd.dlogits', ref['dlogits'], mag['dlogits'], f32['dlogits'], dict(drop_last_term=drop['dlogits']))]


def calibrate_sumsq(count):
    g = R.sumsq_inputs(count, 'decades')
    ref, mag = R.sumsq(g)
    f32, _ = R.sumsq(g, dtype=F32)
    drop, _ = R.sumsq(g, perturb='drop_last_term')
    return [_cal('sumsq.out', ref['out'], mag['out'], f32['out'], dict(drop_last_term=drop['out']))]


def span_buffer(name, family='decades'):
    spans, n = R.SPAN_TABLES[name]
    g = R.sumsq_inputs(n, family)
    if family == 'decades':
        g[spans[-1][0] + spans[-1][1] - 1] = g[-1]     # the last element of the last span carries the largest magnitude
        g[-1] = 1.0
    return spans, g


def calibrate_sumsq_spans(name):
    spans, g = span_buffer(name)
    ref, mag = R.sumsq_spans(g, spans)
    f32, _ = R.sumsq_spans(g, spans, dtype=F32)
    drop, _ = R.sumsq_spans(g, spans, perturb='drop_last_term')
    return [_cal('sumsq_spans.out', ref['out'], mag['out'], f32['out'], dict(drop_last_term=drop['out']))]


def adamw_kw(c):
    return dict(grad_scale=c['gs'], max_norm=c['max_norm'], lr=c['lr'], wd=c['wd'], step=c['step'], decoupled=c['decoupled'])


def calibrate_adamw(c):
    """the GPU test's two consecutive steps; the second starts from the f32 restatement's own state, as the kernel's will from its own"""
    i = R.adamw_inputs(c['count'])
    ss = R.sumsq(i['g'])[0]['out'].float()
    coef = float(R.clip_coef(ss, c['gs'], c['max_norm'])[1])
    state, rows = (i['p'], i['m'], i['v']), []
    for step in (c['step'], c['step'] + 1):
        a, kw = (state[0], i['g'], state[1], state[2], ss), dict(adamw_kw(c), step=step)
        ref, mag = R.adamw(*a, **kw)
        f32, _ = R.adamw(*a, dtype=F32, **kw)
        pert = {k: R.adamw(*a, perturb=k, **kw)[0] for k in R.ADAMW_PERTURB if R.adamw_perturb_applies(k, dict(c, step=step), coef)}
        rows.append(_cal('adamw.p', ref['p'], mag['p'], f32['p'], {k: v['p'] for k, v in pert.items()}))
        rows.append(_cal('adamw.m', ref['m'], mag['m'], f32['m'], {k: v['m'] for k, v in pert.items() if k in ('coupled_for_decoupled', 'no_clip')}))
        rows.append(_cal('adamw.v', ref['v'], mag['v'], f32['v'], {k: v['v'] for k, v in pert.items() if k in ('coupled_for_decoupled', 'no_clip')}))
        rows.append(_cal('adamw.norm', ref['norm'], mag['norm'], f32['norm'], {}))
        state = (f32['p'], f32['m'], f32['v'])
    return rows


def calibrate_adamw_spans(name, step, gs, max_norm, decoupled, wd):
    spans, n = R.SPAN_TABLES[name]
    i = R.adamw_inputs(n, seed=11)
    ss = R.sumsq_spans(i['g'], spans)[0]['out'].float()
    a, kw = (i['p'], i['g'], i['m'], i['v'], spans, ss), dict(step=step, grad_scale=gs, max_norm=max_norm, decoupled=decoupled, wd=wd)
    ref, mag = R.adamw_spans(*a, **kw)
    f32, _ = R.adamw_spans(*a, dtype=F32, **kw)
    one = [(o, n_, 0) for o, n_, _ in spans]        # perturbed: every span at the global step
    pert, _ = R.adamw_spans(i['p'], i['g'], i['m'], i['v'], one, ss, **kw)
    return [_cal('adamw.' + k, ref[k], mag[k], f32[k], dict(span_step_offset_ignored=pert[k]) if k == 'p' else {}) for k in ('p', 'm', 'v')]


def calibrate_clip(count, max_norm):
    i = R.adamw_inputs(count, seed=5)
    ss = R.sumsq(i['g'])[0]['out'].float()
    ref, mag = R.clip_scale(i['g'], ss, max_norm)
    f32, _ = R.clip_scale(i['g'], ss, max_norm, dtype=F32)
    coef = float(R.clip_coef(ss, 1.0, max_norm)[1])
    pert = dict(no_clip=R.clip_scale(i['g'], ss, max_norm, perturb='no_clip')[0]['g']) if coef < 0.5 else {}
    return [_cal('clip_scale.g', ref['g'], mag['g'], f32['g'], pert), _cal('clip_scale.norm', ref['norm'], mag['norm'], f32['norm'], {})]


def _assert_rows(rows):
    for name, f32, pert in rows:
        print(f'CAL {name} f32 {f32:.3g} ' + ' '.join(f'{k} {v:.3g}' for k, v in pert.items()))
    for name, f32, pert in rows:
        assert f32 <= C[name] / 4, (name, 'f32 restatement', f32, C[name])
        for k, v in pert.items():
            assert v >= 2 * C[name], (name, k, v, C[name])


@pytest.mark.parametrize('c', R.HEAD_CASES, ids=R.head_id)
def test_constants_head_fwd(c):
    _assert_rows(calibrate_head_fwd(c))


@pytest.mark.parametrize('c', R.HEAD_CASES + R.HEAD_BWD_B_CASES, ids=R.head_id)
def test_constants_head_bwd(c):
    _assert_rows(calibrate_head_bwd(c))


@pytest.mark.parametrize('case', R.BCE_FWD_CASES, ids=str)
def test_constants_bce_fwd(case):
    _assert_rows(calibrate_bce_fwd(*case[:3]))


@pytest.mark.parametrize('case', R.BCE_BWD_CASES, ids=str)
def test_constants_bce_bwd(case):
    _assert_rows(calibrate_bce_bwd(*case))


@pytest.mark.parametrize('count', R.SUMSQ_COUNTS)
def test_constants_sumsq(count):
    rows = calibrate_sumsq(count)
    if count == 1:
        rows = [(n, f, {}) for n, f, _ in rows]     # one element: nothing is left of the sum without it, trivially far away
    _assert_rows(rows)


@pytest.mark.parametrize('name', list(R.SPAN_TABLES))
def test_constants_sumsq_spans(name):
    _assert_rows(calibrate_sumsq_spans(name))


@pytest.mark.parametrize('c', R.ADAMW_CASES, ids=R.adamw_id)
def test_constants_adamw(c):
    _assert_rows(calibrate_adamw(c))


@pytest.mark.parametrize('case', R.ADAMW_SPAN_CASES, ids=str)
def test_constants_adamw_spans(case):
    _assert_rows(calibrate_adamw_spans(*case))


@pytest.mark.parametrize('case', R.CLIP_CASES, ids=str)
def test_constants_clip_scale(case):
    _assert_rows(calibrate_clip(*case))


# ===================================================================================================================== the exact families
@pytest.mark.parametrize('case', R.HEAD_EXACT_CASES, ids=str)
def test_exact_family_is_exact_in_f32(case):
    """the integer family's f64 results are integers (dX: multiples of rstd / d) that f32 holds exactly, so any summation order gives them"""
    B, N, d, K, _ = case
    i = R.head_exact_inputs(B, d, K)
    a = (i['dl'], i['xhat'], i['rstd'], i['gamma'], i['beta'], i['W'])
    ref, mag = R.head_bwd(*a)
    for k in ('dW', 'dbias', 'dgamma', 'dbeta'):
        assert torch.equal(ref[k], ref[k].round()) and float(mag[k].max()) < 2 ** 24, k
        assert torch.equal(ref[k].float().double(), ref[k])
    if d & (d - 1) == 0:
        assert torch.equal(ref['dX'].float().double(), ref['dX']) and float(mag['dX'].max()) * d < 2 ** 24
        assert torch.equal(R.head_bwd(*a, dtype=F32)[0]['dX'].double(), ref['dX'])


def test_integer_sumsq_is_exact():
    for count in R.SUMSQ_COUNTS:
        g = R.sumsq_inputs(count, 'ints')
        ref, _ = R.sumsq(g)
        assert float(ref['out']) == float(ref['out'].round()) < 2 ** 24
        assert float(R.sumsq(g, dtype=F32)[0]['out']) == float(ref['out'])


def test_grad_accumulate_forms():
    g = torch.Generator().manual_seed(1)
    acc, gr = torch.randn(1000, generator=g), torch.randn(1000, generator=g)
    for mode in (0, 1, 2):
        two, one = R.grad_accumulate(acc, gr, mode, 1.0)
        assert torch.equal(two, one) and torch.equal(two, gr if mode == 0 else gr + acc)     # scale = 1: exact product, one rounding
        two, one = R.grad_accumulate(acc, gr, mode, 0.3)
        assert (mode == 0) == torch.equal(two, one)     # scale = 0.3: the two forms differ somewhere in 1000 elements
