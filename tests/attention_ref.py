"""
A plain torch restatement of the fused bf16 attention contract (include/ecgvit_hip.h and the header comment of csrc/attention_varlen.hip; not the
kernel bodies), with the case lists and input generators that tests/test_attention_ref.py (CPU) and tests/test_gpu_attention_ref.py (MI355X)
share.  The method is that of tests/head_opt_ref.py, whose `ratio` this module imports.

`attention(..., dtype=F64)` is the reference.  `attention(..., dtype=BF16)` is the bf16-staged restatement that calibrates the tolerances: f32
scores and LSE, and the rounding points of the contract -- the forward's probabilities go to bf16 before P V; the backward rebuilds P from the f32
LSE and rounds it to bf16 (for dV), rounds dS to bf16 (for dQ, dK), takes delta = sum_j dO_j O_j from the stored bf16 `out`, and stores bf16
results; at dh = 64 and more than 256 tokens (uniform entry points) dQ is re-rounded to bf16 after every 256-key window ("each window after the
first adding its dQ to the bf16 dQ already in dqkv").

Both return (out, mag): dicts name -> tensor for out, lse, dQ, dK, dV and probs.  mag[name] is the sum of the absolute terms of the final
expression of out[name], in float64, with P~ = P mult (mult: the dropout multipliers [B,h,N,N]):

    out   sum_k P~ |v|                          dV   sum_q P~ |dO|
    dS    T = P (|dP| + sum_j |dO_j O_j|)       dK   scale sum_q T |q|        dQ   scale sum_k T |k|
    lse   |lse| + max_k |s|                     probs   P (1 + |s| + |lse|)

Errors are judged element by element as ratio = |got - ref| / (u mag), never relative to |ref|: u = 2^-9 for the bf16 results, after the half
bf16 ulp of the reference that `head_opt_ref.ratio(..., bf16_out=True)` allows, and u = 2^-24 for the f32 results lse and probs.

Input families: 'randn' (randn 1.5) and 'planted' (see `record_inputs`): groups of edge queries and edge keys share one coordinate, so that an
edge query puts most of its mass on the few edge keys of its groups -- a (query, key) pair dropped at an edge is then a large part of a row, not
1 / N of it.  'rising', 'falling' and 'spike' are the score profiles of test_attention_fwd_lazy_running_maximum, for the forward only.

`perturb=` names one wrong kernel each (PERTURBATIONS); C[name] is chosen so that, on every case the GPU file runs, the bf16-staged
restatement's worst ratio is <= C / 4 and every applicable perturbation lies >= 2 C away on the outputs it is held on (test_attention_ref.py
proves both).  Worst / nearest over the case lists; `MI355X` = the kernels, measured by tests/test_gpu_attention_ref.py:

    name        C    restatement   nearest perturbation                          MI355X
    out      16       1.78          52.3 drop_window_first_key                  1.77
    lse      64       9.35             - (no perturbation is held on it)      9.35
    dQ       16       3.89          52.3 dq_miss_last_key_one_block             3.89
    dK       16       2.98          40.3 delta_from_undropped_out               2.11
    dV       16       1.98           137 dkdv_miss_last_query_last_tile         1.65
    probs    64       10.7             - (no perturbation is held on it)      5.51

(restatement, by case list, out / lse / dQ / dK / dV: uniform dh 64 1.56, 2.15, 3.89, 1.70, 1.26; uniform dh 128 1.61, 5.29, 1.23, 1.31, 1.33; many
items 1.60, 1.63, 2.01, 1.26, 1.25; variable length 1.45, 9.35, 1.52, 1.25, 1.33; CLS rows 1.30, 9.35, 1.15, 2.98, 1.98; dropout 1.78, 3.51, 3.18,
2.52, 1.88.  MI355X, the same: uniform dh 64 1.77, 4.41, 3.89, 2.11, 1.26; uniform dh 128 1.67, 2.84, 1.75, 1.21, 1.33; many items 1.64, 1.86, 2.44,
1.26, 1.25; variable length 1.70, 9.35, 1.85, 1.45, 1.65; dropout 1.76, 2.42, 1.82, 1.23, 1.24; the CLS-row kernels keep f32 to the end: out 4e-4,
lse 9.35, dQ 0.70, dK 1.37, dV 1.3e-3.  The dQ figure is the bf16 re-rounding after each of eight key windows at 2048 tokens, the lse figure the
f32 score of a one-token record at dh = 128: the kernels and the restatement round the same values there.)  A perturbation is counted on the
output of its list (PERTURBATIONS) that shows it best; the forward ones are held on `out` alone, where they are weakest (on lse they lie 1e4
and more away).  A uniform case is calibrated over the records the GPU test holds, a variable-length case one record at a time: each length
is a shape of its own, for the full kernels and for the CLS row.

Where a perturbation coincides with the reference by construction it is not asked to lie 2 C away (`applies`): a one-token record has no key
to drop; the window perturbations need a second 256-key window; the dropout ones need dropout; `mask_index_uses_n_tok` and `include_pad_key`
need a record shorter than the batch; `head_stride_dh64` needs dh = 128; the CLS row is in the last 32-query block only up to 32 tokens.  The
perturbations that drop one (query, key) pair at an edge, and the delta that skips its last column, are asked for on the planted family only
(EDGE_PAIR): under i.i.d. inputs such a pair carries about 1 / N of a row and lies below the rounding noise by construction (as low as 1.0 on the
randn cases of 1025 tokens).  On the planted family every one of them separates at every shape and every record length of the case
lists, the one-key last tiles of 129, 257, 513 and 1025 tokens included.  The planted family alone would hide an error on an interior key of
an edge query (the CLS row is one: its mass sits on about four keys), so every case list runs both families.
"""
import math

import torch

from head_opt_ref import ratio, F64, F32, BF16

U_BF16_OVER_U_F32 = 2.0 ** 15      # ratio() counts in u = 2^-24; a bf16 result's unit is 2^-9

# name -> C.  The measurements behind them are in the table of the module docstring.
C = {'out': 16.0, 'lse': 64.0, 'dQ': 16.0, 'dK': 16.0, 'dV': 16.0, 'probs': 64.0}

PERTURBATIONS = {   # name -> the outputs it is held on
    'drop_last_key': ('out',),
    'drop_window_first_key': ('out',),
    'include_pad_key': ('out',),
    'dq_miss_last_key_one_block': ('dQ',),
    'dkdv_miss_last_query_last_tile': ('dK', 'dV'),
    'delta_from_undropped_out': ('dQ', 'dK'),
    'delta_skips_last_col': ('dQ', 'dK'),
    'scale_missing_on_dk': ('dK',),
    'mask_index_uses_n_tok': ('out', 'dV'),
    'head_stride_dh64': ('out',),
    'dq_window_not_accumulated': ('dQ',),
}
BF16_OUTPUTS = ('out', 'dQ', 'dK', 'dV')
# one (query, key) pair at an edge: under i.i.d. inputs such a pair carries about 1 / N of a row, below the rounding noise by construction, so these
# are asked to lie 2 C away on the planted family only; delta_skips_last_col leans on that family's heavy last column in the same way
EDGE_PAIR = ('drop_last_key', 'drop_window_first_key', 'include_pad_key', 'dq_miss_last_key_one_block', 'dkdv_miss_last_query_last_tile',
             'delta_skips_last_col')


def judge(name, got, ref, mag):
    """worst ratio of one output in its own unit"""
    mag = mag.detach().double().cpu()
    if name in BF16_OUTPUTS:
        return ratio(got, ref, mag * U_BF16_OVER_U_F32, bf16_out=True)
    return ratio(got, ref, mag)


# ===================================================================================================================== restatement
def _one(q, k, v, do, scale, staged, mult, perturb, dq_windows, probs):
    """one record: q, do [h, nq, dh]; k, v [h, nk, dh]; mult [h, nq, nk] or None.  nq < nk only for the CLS row (nq = 1) and a counted pad key"""
    W = F32 if staged else F64
    rb = (lambda t: t.to(BF16).to(W)) if staged else (lambda t: t)
    q, k, v, do = (t.to(W) for t in (q, k, v, do))
    nq, nk = q.shape[1], k.shape[1]
    if perturb == 'head_stride_dh64':
        v = torch.cat([v[..., :64], v[..., :64]], -1)
    s = (q @ k.transpose(1, 2)) * scale
    # ---- forward
    sf = s
    if perturb == 'drop_last_key':
        sf = s.clone()
        sf[:, 32 * ((nq - 1) // 32):, nk - 1] = -math.inf
    if perturb == 'drop_window_first_key':
        sf = s.clone()
        sf[:, :32, 256 * ((nk - 1) // 256)] = -math.inf
    m = sf.max(-1, keepdim=True).values
    e = torch.exp(sf - m)
    l = e.sum(-1, keepdim=True)
    lse = (m + torch.log(l))[..., 0]
    out = rb((rb(e if mult is None else e * mult) @ v) / l)
    # ---- backward, from the stored out and lse
    P = torch.exp(s - lse[..., None])
    Pt = P if mult is None else P * mult
    dP = do @ v.transpose(1, 2)
    if mult is not None:
        dP = dP * mult
    o_delta = rb(P @ v) if perturb == 'delta_from_undropped_out' else out
    dd = do * o_delta
    delta = (dd[..., :-1] if perturb == 'delta_skips_last_col' else dd).sum(-1, keepdim=True)
    dS, PtR = rb(P * (dP - delta)), rb(Pt)
    dSk, Ptk = dS, PtR
    if perturb == 'dkdv_miss_last_query_last_tile':
        dSk, Ptk = dS.clone(), PtR.clone()
        dSk[:, nq - 1, 32 * ((nk - 1) // 32):] = 0
        Ptk[:, nq - 1, 32 * ((nk - 1) // 32):] = 0
    dV = rb(Ptk.transpose(1, 2) @ do)
    dK = rb(dSk.transpose(1, 2) @ q * (1.0 if perturb == 'scale_missing_on_dk' else scale))
    dSq = dS
    if perturb == 'dq_miss_last_key_one_block':
        dSq = dS.clone()
        dSq[:, :32, nk - 1] = 0
    if dq_windows and nk > 256:
        dQ = torch.zeros_like(q)
        for k0 in range(0, nk, 256):
            part = dSq[:, :, k0:k0 + 256] @ k[:, k0:k0 + 256] * scale
            dQ = rb(part if k0 == 0 or perturb == 'dq_window_not_accumulated' else dQ + part)
    else:
        dQ = rb(dSq @ k * scale)
    res = dict(out=out, lse=lse, dQ=dQ, dK=dK, dV=dV)
    A = lambda t: t.double().abs()
    P6, Pt6 = P.double(), Pt.double()
    T = P6 * (A(dP) + A(do * out).sum(-1, keepdim=True))
    mag = dict(out=Pt6 @ A(v), lse=A(lse) + A(s).max(-1).values, dQ=scale * (T @ A(k)), dK=scale * (T.transpose(1, 2) @ A(q)),
               dV=Pt6.transpose(1, 2) @ A(do))
    if probs:
        res['probs'], mag['probs'] = P, P6 * (1.0 + A(s) + A(lse)[..., None])
    return res, mag


def attention(qkv, do, B, N, h, dh, dtype=F64, n_tok=None, mult=None, perturb=None, cls=False, dq_windows=None, probs=False):
    """qkv [B*N, 3 h dh] (columns [q | k | v], head-major inside each), do [B*N, h dh] (cls: [B, h dh], the upstream gradient of row 0), n_tok a
    list of B lengths or None, mult [B,h,N,N] or None.  Returns out, dQ, dK, dV [B, N, h dh], lse [B, h, N], probs [B, h, N, N] (cls: out, dQ
    [B, h dh], lse [B, h]); rows >= n_tok[b] are zeros, their lse 0.  dq_windows: dQ is re-rounded after every 256-key window (default: dh = 64,
    uniform, full rows).  perturb 'mask_index_uses_n_tok' expects the wrong multipliers in `mult`."""
    staged = dtype == BF16
    W = F32 if staged else F64
    scale = float(torch.tensor(dh ** -0.5, dtype=F32))
    if dq_windows is None:
        dq_windows = dh == 64 and n_tok is None and not cls
    d = h * dh
    x = qkv.reshape(B, N, 3, h, dh).permute(2, 0, 3, 1, 4)       # [3, B, h, N, dh]
    g = do.reshape(B, 1 if cls else N, h, dh).permute(0, 2, 1, 3)
    nq_all = 1 if cls else N
    dev = qkv.device
    res = dict(out=torch.zeros(B, nq_all, d, dtype=W, device=dev), lse=torch.zeros(B, h, nq_all, dtype=W, device=dev),
               dQ=torch.zeros(B, nq_all, d, dtype=W, device=dev), dK=torch.zeros(B, N, d, dtype=W, device=dev), dV=torch.zeros(B, N, d, dtype=W, device=dev))
    mag = {k_: torch.zeros(t.shape, dtype=F64, device=dev) for k_, t in res.items()}
    if probs:
        res['probs'], mag['probs'] = torch.zeros(B, h, N, N, dtype=W, device=dev), torch.zeros(B, h, N, N, dtype=F64, device=dev)
    unheads = lambda t: t.permute(1, 0, 2).reshape(t.shape[1], d)
    for b in range(B):
        n = N if n_tok is None else int(n_tok[b])
        nq = 1 if cls else n
        nk = n + 1 if perturb == 'include_pad_key' and n < N else n
        mb = None if mult is None else mult[b, :, :nq, :nk].to(W)
        r, m_ = _one(x[0, b, :, :nq], x[1, b, :, :nk], x[2, b, :, :nk], g[b, :, :nq], scale, staged, mb, perturb, dq_windows, probs)
        for src, dst in ((r, res), (m_, mag)):
            dst['out'][b, :nq], dst['dQ'][b, :nq] = unheads(src['out']), unheads(src['dQ'])
            dst['dK'][b, :n], dst['dV'][b, :n] = unheads(src['dK'][:, :n]), unheads(src['dV'][:, :n])
            dst['lse'][b, :, :nq] = src['lse']
            if probs:
                dst['probs'][b, :, :nq, :n] = src['probs'][:, :, :n]
    if cls:
        for dct in (res, mag):
            dct['out'], dct['dQ'], dct['lse'] = dct['out'][:, 0], dct['dQ'][:, 0], dct['lse'][:, :, 0]
    return res, mag


# ===================================================================================================================== inputs and cases
BOOST = 12.0      # score a planted (query, key) pair gains: e^12 against the e^0.5 N of the rest of a row


def edge_groups(n, N):
    """[(coordinate, queries, keys)] of a record of n tokens in a batch of N: the ends group {0, n-2, n-1} with the last 256-key window's first
    key and the first pad key n (never a query); one group per 32-tile edge 32 j: {32 j - 1, 32 j, 32 j + 1}.  127/128, 255/256 and 511/512 are
    tile edges"""
    ends = sorted({0, max(n - 2, 0), n - 1})
    groups = [(0, ends, sorted(set(ends) | {256 * ((n - 1) // 256)} | ({n} if n < N else set())))]
    for j in range(1, (n - 1) // 32 + 1):
        mem = [t for t in (32 * j - 1, 32 * j, 32 * j + 1) if t < n]
        groups.append((j, mem, mem))
    return groups


def record_inputs(seed, N, h, dh, family='randn', n=None):
    """(qkv [N, 3 h dh], do [N, h dh]) of one record, f32 holding bf16 values.  Rows >= n (pad) hold values as large as the valid ones"""
    n = N if n is None else n
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 3, h, dh, generator=g) * (1.0 if family == 'planted' else 1.5)
    do = torch.randn(N, h * dh, generator=g)
    if family == 'planted':
        a = math.sqrt(BOOST * math.sqrt(dh))
        for c, qs, ks in edge_groups(n, N):
            x[qs, 0, :, c] = a
            x[ks, 1, :, c] = a
        x[:, 2, :, dh - 1] *= 8.0       # a heavy last column of V and dO: the term a delta that stops at dh - 2 leaves out
        do.view(N, h, dh)[:, :, dh - 1] *= 8.0
        # the ends group's gradient is not left to chance (the CLS row is one query): its queries carry dO = 8 in that column and its keys
        # 0 and n - 1 the values 4 and 12, so dP - delta = 8 (v - O) stays far from zero on key n - 1 and dO O on the last column is large
        ends = edge_groups(n, N)[0][1]
        do.view(N, h, dh)[ends, :, dh - 1] = 8.0
        x[0, 2, :, dh - 1] = 4.0
        x[n - 1, 2, :, dh - 1] = 12.0
    elif family in ('rising', 'falling'):
        ramp = torch.linspace(0.2, 6.0, N).view(N, 1, 1)
        x[:, 1] *= ramp if family == 'rising' else ramp.flip(0)
    elif family == 'spike':
        x[max(n - 40, 0), 1] *= 25.0
    return x.reshape(N, 3 * h * dh).to(BF16).float(), do.to(BF16).float()


def case(N, dh=64, B=2, h=2, family='randn', lengths=None, p=0.0, cls=False):
    return dict(N=N, dh=dh, B=B, h=h, family=family, lengths=lengths, p=p, cls=cls)


def case_id(c):
    return (f"N{c['N']}-dh{c['dh']}-B{c['B']}-h{c['h']}-{c['family']}" + ('-varlen' if c['lengths'] else '') + (f"-p{c['p']:g}" if c['p'] else '')
            + ('-cls' if c['cls'] else ''))


def varlen_lengths(N):
    return [1, 32, 33, 128, 129, N - 1, N]


def case_records(c):
    """the records of a case that are held against fp64: first, middle and last (every record of a variable-length case: each length is a case)"""
    B = c['B']
    return list(range(B)) if c['lengths'] else sorted({0, B // 2, B - 1})


def case_inputs(c, recs=None):
    """(qkv [R*N, 3 h dh], do [R*N, h dh] or [R, h dh] for a CLS case) of the records `recs` (default: all) of a case"""
    recs = range(c['B']) if recs is None else recs
    N, h, dh = c['N'], c['h'], c['dh']
    parts = [record_inputs(100003 * N + 1009 * dh + 17 * h + b, N, h, dh, c['family'], c['lengths'][b] if c['lengths'] else None) for b in recs]
    qkv, do = torch.cat([p_[0] for p_ in parts]), torch.cat([p_[1] for p_ in parts])
    if c['cls']:
        do = do.view(len(parts), N, h * dh)[:, 0].contiguous()
    return qkv, do


FAMILIES = ('randn', 'planted')
N_DH64 = [1, 33, 128, 129, 256, 257, 512, 513, 1025, 2048]
N_DH128 = [1, 64, 65, 128, 129, 257, 2048]
UNIFORM_CASES = ([case(N, 64, 3 if N <= 513 else 1, 2, f) for N in N_DH64 for f in FAMILIES]
                 + [case(N, 128, 3 if N <= 257 else 1, 2, f) for N in N_DH128 for f in FAMILIES])
# more than 768 items: a persistent backward workgroup walks several items in both launches; >= 256 items at 300 tokens: the streamed forward;
# >= 256 items of (record, head, 512-query block) at 1025 tokens: the forward's 512-query-block form
MANY_ITEM_CASES = [case(N, 64, B, 2, f) for N, B in ((257, 385), (300, 130), (1025, 64)) for f in FAMILIES]
VARLEN_CASES = [case(N, dh, 7, 2, f, varlen_lengths(N)) for dh in (64, 128) for N in (257, 1025) for f in FAMILIES]
# the CLS-row kernels at the lengths of the full kernels
CLS_CASES = ([case(N, dh, 2, 2, f, cls=True) for dh, Ns in ((64, N_DH64), (128, N_DH128)) for N in Ns for f in FAMILIES]
             + [case(N, dh, 7, 2, f, varlen_lengths(N), cls=True) for dh in (64, 128) for N in (257, 1025) for f in FAMILIES])
DROPOUT_P = 0.1
DROPOUT_CASES = ([case(N, 64, 2, 2, f, p=DROPOUT_P) for N in (129, 257, 513) for f in FAMILIES] + [case(129, 128, 2, 2, f, p=DROPOUT_P) for f in FAMILIES]
                 + [case(257, 64, 7, 2, f, varlen_lengths(257), p=DROPOUT_P) for f in FAMILIES]
                 + [case(129, 64, 2, 2, f, p=DROPOUT_P, cls=True) for f in FAMILIES])
PROFILE_CASES = [case(N, 64, 2, 3, f) for N in (251, 501) for f in ('rising', 'falling', 'spike')]      # forward only
PROBS_CASES = [case(N, dh, 2, 2, f) for N in (33, 257) for dh in (64, 128) for f in FAMILIES]


def cpu_mult(B, h, N, p, seed, recs, lengths=None):
    """dropout multipliers [len(recs), h, N, N] with the statistics of the contract's (one 8-bit draw per key, four keys per 32-bit word, keep iff
    byte >= round(256 p), kept values scaled by 256 / (256 - round(256 p))), from torch's generator -- the calibration needs a realisation, not
    the kernels' hash.  The word of element (bh, q, key) is (bh S + q) ceil(S / 4) + key / 4 with S = N; `lengths` gives the wrong kernel of
    'mask_index_uses_n_tok', S = n_tok[b]"""
    t = round(256 * p)
    nw = B * h * N * ((N + 3) // 4)
    keep = (torch.randint(0, 256, (nw, 4), generator=torch.Generator().manual_seed(seed)) >= t).reshape(-1)
    out = []
    for b in recs:
        S = N if lengths is None else lengths[b]
        bh = (b * h + torch.arange(h)).view(h, 1, 1)
        q, key = torch.arange(N).view(1, N, 1), torch.arange(N).view(1, 1, N)
        word = ((bh * S + q) * ((S + 3) // 4) + key // 4) % nw
        out.append(keep[word * 4 + key % 4])
    return torch.stack(out).double() * (256.0 / (256.0 - t))


def applies(name, c, n):
    """does perturbation `name` differ from the reference by construction on a record of n tokens of case c"""
    N = c['N']
    if name in EDGE_PAIR and c['family'] != 'planted':
        return False
    if name == 'drop_last_key':
        return n >= 2 and (not c['cls'] or n <= 32)          # the last 32-query block: holds row 0 only up to 32 tokens
    if name in ('drop_window_first_key', 'dq_window_not_accumulated'):
        if name == 'dq_window_not_accumulated' and (c['dh'] != 64 or c['lengths'] or c['cls']):
            return False
        return n > 256
    if name == 'include_pad_key':
        return bool(c['lengths']) and n < N
    if name == 'dq_miss_last_key_one_block':
        return n >= 2
    if name == 'dkdv_miss_last_query_last_tile':
        return n >= 2 and (not c['cls'] or 32 * ((n - 1) // 32) == 0)    # the CLS row is the last query only of a one-token record
    if name == 'delta_from_undropped_out':
        return c['p'] > 0 and n >= 2
    if name == 'delta_skips_last_col':
        return n >= 2                                    # one key: P = 1 and dS = P (dP - delta) is held by its terms, both kinds are one product
    if name == 'scale_missing_on_dk':
        return n >= 2
    if name == 'mask_index_uses_n_tok':
        return c['p'] > 0 and bool(c['lengths']) and 4 <= n < N
    if name == 'head_stride_dh64':
        return c['dh'] == 128
    raise KeyError(name)
