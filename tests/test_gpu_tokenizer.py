"""GPU: the segment tokenizer's kernels (csrc/tokenize.hip) and `EcgTokenizer` against the f64 restatement (tests/tokenizer_ref.py) and the
fixture the reference wrote (tests/golden/tokenizer.npz).

Bounds (u = 2^-24, x the raw padded segment, s = x - mean):
  mean   |mean32 - mean64| <= k u mean|x|: k - 1 additions, each rounding at most u times a partial sum of at most sum|x|, then an exact * 1/k.
  choice d64(chosen) - d64(best) <= 64 u (|x|^2 + |c_chosen|^2 + |c_best|^2): k + 3 roundings of at most the bracket in each of the two
         scores plus the f32 mean's shift, a factor of about 2 to spare at k = 32.
  dist   |dist32 - d64(chosen)| <= 4 (k + 2) u (|x|^2 + |c|^2): k + 2 roundings of at most d <= 2 (|s|^2 + |c|^2) <= 2 (|x|^2 + |c|^2), and the
         mean's shift delta <= k u mean|x| moves d by 2 delta sum|s - c| <= k u (|x|^2 + d).
  centre |c32 - c64| <= 1e-6 max|c_j| per centre (the issue's figure): the fixed-point sums round at A 2^-31 per sample, the rest is the f32
         mean of each segment and the final rounding to f32."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import ecg_representation_learning_amd as E
import tokenizer_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
DEV = 'cuda'


def encode(tok, sig, table, offsets=None, idxs=None, dense=False):
    """ids, means, dist straight from the assign kernel (the public call does not return dist) -> tensors of the store's output shape"""
    st = tok._dense_store(sig) if dense else tok._record_store(sig, offsets, idxs)
    ids, means, dist = st.new(torch.int32), st.new(torch.float32), st.new(torch.float32)
    tok._assign(st, table, ids, means, dist=dist)
    torch.cuda.synchronize()
    return ids, means, dist, st


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def zero_mean_centers(rng, V, k):
    c = rng.standard_normal((V, k))
    return (c - c.mean(axis=1, keepdims=True)).astype(np.float32)


def check_choice(sig, k, mode, centers, ids, means, dist=None, ids_best=None, label=''):
    """the bounds of the module docstring for one encode of `sig` (numpy f32 (..., L)); returns the share of segments off the f64 argmin"""
    raw = R.pad(sig.astype(np.float64), k, mode).reshape(-1, k)
    segs, means64 = R.segments(sig, k, mode)
    c64 = centers.astype(np.float64)
    ids = ids.reshape(-1).astype(np.int64)
    assert ids.min() >= 0 and ids.max() < len(centers)
    if ids_best is None:
        ids_best, _ = R.nearest(segs, c64)
    merr = np.abs(means.reshape(-1).astype(np.float64) - means64)
    mbound = k * U * np.abs(raw).mean(axis=1)
    d_ch, d_b = R.dist_to(segs, c64, ids), R.dist_to(segs, c64, ids_best)
    cn = (c64 ** 2).sum(-1)
    x2 = (raw ** 2).sum(-1)
    bound = 64 * U * (x2 + cn[ids] + cn[ids_best])
    share = float((ids != ids_best).mean())
    print(f'{label}: off the f64 argmin {share:.2e}; worst (d_chosen - d_best) / bound {float(((d_ch - d_b) / bound).max()):.3f}; '
          f'worst mean error / bound {float((merr / np.maximum(mbound, 1e-300)).max()):.3f}')
    assert np.all(merr <= mbound)
    assert np.all(d_ch - d_b <= bound)
    if dist is not None:
        dbound = 4 * (k + 2) * U * (x2 + cn[ids])
        derr = np.abs(dist.reshape(-1).astype(np.float64) - d_ch)
        print(f'{label}: worst dist error / bound {float((derr / dbound).max()):.3f}')
        assert np.all(derr <= dbound)
    return share


# ---- 1. layouts -----------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,lengths', [('shift', [61, 8, 16, 257, 33]), ('zero', [61, 8, 16, 257, 33, 1, 3])])
def test_layouts_give_the_same_bits(mode, lengths):
    rng = np.random.default_rng(11)
    k, V = 8, 300
    centers = zero_mean_centers(rng, V, k)
    tok = E.EcgTokenizer.from_centers(centers, np.ones(V, np.int64), pad=mode)
    table = tok._table(torch.device(DEV, torch.cuda.current_device()), None)
    recs = [rng.normal(0.3, 0.7, (12, l)).astype(np.float32) for l in lengths]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    S = int(off[-1])
    # the canon: every record on its own as a dense (12, l) tensor
    canon = []
    for rec in recs:
        ids, means, dist, _ = encode(tok, torch.from_numpy(rec).to(DEV), table, dense=True)
        T = rec.shape[1] // k + 1
        canon.append((ids.view(12, T), means.view(12, T), dist.view(12, T)))
        check_choice(rec, k, mode, centers, ids.cpu().numpy(), means.cpu().numpy(), dist.cpu().numpy(), label=f'{mode} l={rec.shape[1]}')
    ids2, means2 = tok(torch.from_numpy(recs[0]).to(DEV))          # the public call is the same launch
    assert same_bits(ids2, canon[0][0]) and same_bits(means2, canon[0][1])
    want = [torch.cat([c[j] for c in canon], dim=1) for j in range(3)]
    flat = np.concatenate(recs, axis=1)
    sel = [0, 3, 4]
    want_sel = [torch.cat([canon[i][j] for i in sel], dim=1) for j in range(3)]
    for shift in (0, 1, 2, 3):                                       # a ragged store whose first sample sits 0..3 floats past a 16-byte boundary
        buf = torch.zeros(12 * S + 4, dtype=torch.float32, device=DEV)
        store = buf[shift:shift + 12 * S].view(12, S)
        store.copy_(torch.from_numpy(flat))
        assert store.data_ptr() % 16 == 4 * shift and store.is_contiguous()
        ids, means, dist, st = encode(tok, store, table, offsets=off)
        assert ids.shape == (12, sum(l // k + 1 for l in lengths))
        assert same_bits(ids, want[0]) and same_bits(means, want[1]) and same_bits(dist, want[2]), shift
        ids, means, dist, _ = encode(tok, store, table, offsets=off, idxs=sel)
        assert same_bits(ids, want_sel[0]) and same_bits(means, want_sel[1]) and same_bits(dist, want_sel[2]), shift
        r_ids, r_means, seg_off = tok(store, offsets=off)
        assert same_bits(r_ids, want[0]) and same_bits(r_means, want[1]) and seg_off.tolist() == st.seg_cum.tolist()
    # a rectangle of equal-length records, whole and in two cuts
    rect = torch.from_numpy(np.stack([recs[0]] + [rng.normal(0.3, 0.7, (12, lengths[0])).astype(np.float32) for _ in range(3)])).to(DEV)
    whole = encode(tok, rect, table)[:3]
    a, b = encode(tok, rect[:1].contiguous(), table)[:3], encode(tok, rect[1:].contiguous(), table)[:3]
    for j in range(3):
        assert whole[j].shape == (4, 12, lengths[0] // k + 1)
        assert same_bits(whole[j], torch.cat([a[j], b[j]])) and same_bits(whole[j][0], canon[0][j])
    sub = encode(tok, rect, table, idxs=[0, 3])[:3]
    for j in range(3):
        assert same_bits(sub[j], whole[j][[0, 3]])


# ---- 2. table shapes --------------------------------------------------------------------------------
@pytest.mark.parametrize('k,V', [(8, 1), (8, 37), (8, 300), (8, 4096), (16, 1000), (32, 4097)])
def test_table_shapes_against_f64(k, V):
    rng = np.random.default_rng(100 * k + V)
    rows, T = 100, 200                                               # 20 000 segments; the last of every row is padded
    L = (T - 1) * k + 5
    sig = rng.normal(0.3, 0.7, (rows, L)).astype(np.float32)
    centers = zero_mean_centers(rng, V, k)
    tok = E.EcgTokenizer.from_centers(centers, np.ones(V, np.int64))
    x = torch.from_numpy(sig).to(DEV)
    ids, means, dist, _ = encode(tok, x, tok._table(x.device, None), dense=True)
    assert ids.numel() == 20000
    share = check_choice(sig, k, 'shift', centers, ids.cpu().numpy(), means.cpu().numpy(), dist.cpu().numpy(), label=f'k={k} V={V}')
    assert share <= 1e-3
    assert torch.equal(x.cpu(), torch.from_numpy(sig))


# ---- planted data ------------------------------------------------------------------------------------
def planted(rng, V, k, n=4, segs_per_row=25):
    """(n, 12, segs_per_row * k) records whose segments are centre j + noise of sigma = 0.02 x the smallest centre spacing + a random DC offset.
    k divides the length, so 'shift' appends a copy of every row's last segment: its planted id is known too."""
    centers = zero_mean_centers(rng, V, k)
    d = R.sqdist(centers.astype(np.float64), centers) + np.eye(V) * 1e30
    spacing = float(np.sqrt(d.min()))
    j = rng.integers(0, V, (n, 12, segs_per_row))
    j.reshape(-1)[:V] = np.arange(V)                                 # every centre has a segment
    noise = rng.standard_normal((n, 12, segs_per_row, k)) * (0.02 * spacing)
    dc = rng.normal(0, 0.5, (n, 12, segs_per_row, 1))
    sig = (centers[j] + noise + dc).astype(np.float32).reshape(n, 12, segs_per_row * k)
    ids = np.concatenate([j, j[..., -1:]], axis=-1)
    return sig, centers, ids


@pytest.fixture(scope='module')
def plant():
    rng = np.random.default_rng(37)
    sig, centers, ids = planted(rng, 37, 8)
    segs, _ = R.segments(sig, 8, 'shift')
    best, _ = R.nearest(segs, centers)
    assert np.array_equal(best, ids.reshape(-1))                     # in f64 every planted id is recovered
    return sig, centers, ids, segs


def centre_close(got, want):
    err = np.abs(got.astype(np.float64) - want).max(axis=1) / np.abs(want).max(axis=1)
    print(f'worst centre error relative to max|c_j|: {float(err.max()):.3e}')
    return bool(np.all(err <= 1e-6))


def run_update(tok, sig, ids, table, offsets=None, ws=None):
    """one update from `table`; ws: the workspace of an earlier update over the same store, whose absolute maximum is used again"""
    st = tok._record_store(sig, offsets, None)
    table = table.clone()
    lens = torch.full((table.shape[0],), -1, dtype=torch.int64, device=sig.device)
    keep = ws is not None
    if ws is None:
        ws = torch.empty(E.hip.lib().ecgvit_tok_workspace(table.shape[0], tok.k) // 8, dtype=torch.int64, device=sig.device)
    tok._update(st, ids, table, lens, ws, keep_amax=keep)
    torch.cuda.synchronize()
    return table, lens, ws


def test_planted_ids_and_update(plant):
    sig, centers, ids, segs = plant
    tok = E.EcgTokenizer.from_centers(centers, np.ones(37, np.int64))
    x = torch.from_numpy(sig).to(DEV)
    got, means = tok(x)
    assert got.shape == (4, 12, 26) and np.array_equal(got.cpu().numpy(), ids)
    start = torch.from_numpy(centers).to(DEV)
    table, lens, _ = run_update(tok, x, got, start)
    want_c, want_l = R.update(segs, ids.reshape(-1), centers)
    assert np.array_equal(lens.cpu().numpy(), want_l) and int(want_l.min()) >= 1
    assert centre_close(table.cpu().numpy(), want_c)


# ---- 4. update on random ids ---------------------------------------------------------------------------
@pytest.mark.parametrize('k,mode', [(8, 'shift'), (16, 'zero'), (32, 'shift')])
def test_update_random_ids(k, mode):
    rng = np.random.default_rng(k)
    n, L, V = 5, 189, 24
    T = L // k + 1
    sig = rng.normal(0.3, 0.7, (n, 12, L)).astype(np.float32)
    ids = rng.integers(0, V, (n, 12, T)).astype(np.int32)
    ids[np.isin(ids, [3, 7, 23])] = 0                                # three centres receive nothing
    start = zero_mean_centers(rng, V, k)
    tok = E.EcgTokenizer(k=k, pad=mode)
    x, d_ids, d_start = torch.from_numpy(sig).to(DEV), torch.from_numpy(ids).to(DEV), torch.from_numpy(start).to(DEV)
    table, lens, ws = run_update(tok, x, d_ids, d_start)
    segs, _ = R.segments(sig, k, mode)
    want_c, want_l = R.update(segs, ids.reshape(-1).astype(np.int64), start)
    assert np.array_equal(lens.cpu().numpy(), want_l) and want_l[[3, 7, 23]].tolist() == [0, 0, 0]
    got = table.cpu().numpy()
    assert np.array_equal(got[[3, 7, 23]], start[[3, 7, 23]])       # unchanged, bit for bit
    live = want_l > 0
    assert centre_close(got[live], want_c[live])
    again, lens2, _ = run_update(tok, x, d_ids, d_start)
    assert same_bits(again, table) and torch.equal(lens2, lens)
    other = torch.where(d_ids == 1, torch.full_like(d_ids, 2), d_ids)      # other ids, the maximum of the first call's workspace used again
    kept, lens_k, _ = run_update(tok, x, other, d_start, ws=ws)
    fresh, lens_f, _ = run_update(tok, x, other, d_start)
    assert same_bits(kept, fresh) and torch.equal(lens_k, lens_f) and int(lens_k[1]) == 0 and not same_bits(kept, table)
    # the same records as a ragged store: record r's samples at columns r L .. (r + 1) L, its segments at columns r T .. (r + 1) T
    store = x.permute(1, 0, 2).reshape(12, n * L).contiguous()
    r_ids = d_ids.permute(1, 0, 2).reshape(12, n * T).contiguous()
    ragged, lens3, _ = run_update(tok, store, r_ids, d_start, offsets=np.arange(n + 1) * L)
    assert same_bits(ragged, table) and torch.equal(lens3, lens)


# ---- 5. fit ------------------------------------------------------------------------------------------
def test_fit_from_a_fixed_start(plant):
    sig, centers, ids, segs = plant
    rng = np.random.default_rng(5)
    init = (centers + rng.standard_normal(centers.shape) * 0.01).astype(np.float32)
    x = torch.from_numpy(sig).to(DEV)
    before = x.clone()
    tok = E.EcgTokenizer(k=8).fit(x, method='kmeans', cls_kwargs=dict(n_clusters=37, init=init, max_iter=16))
    want_c, want_l, _, history = R.lloyd(segs, init, max_iter=16)
    print('changed per iteration:', tok.changed_, 'restatement:', history)
    assert tok.changed_[-1] == 0 and tok.n_iter_ <= 3 and tok.changed_ == history
    assert np.array_equal(tok.lens, want_l) and tok.lens.dtype == np.int64 and centre_close(tok.centers, want_c)
    assert tok.centers.shape == (37, 8) and tok.centers.dtype == np.float32
    assert (tok.fit_method, tok.n_sig, tok.cls_th) == ('kmeans', 4, 37)
    assert torch.equal(x, before)
    got, _ = tok(x)
    assert np.array_equal(got.cpu().numpy(), ids)
    part = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(n_clusters=37, init=init), idxs=[0, 2])
    assert part.n_sig == 2 and int(part.lens.sum()) == 2 * 12 * 26


def test_fit_random_restarts(plant):
    sig = plant[0]
    x = torch.from_numpy(sig).to(DEV)
    kw = dict(n_clusters=37, init='random', random_state=7, max_iter=8)
    one = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(kw, n_init=1))
    two = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(kw, n_init=2))
    again = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(kw, n_init=2))
    assert np.array_equal(two.centers, again.centers) and np.array_equal(two.lens, again.lens) and two.inertia_ == again.inertia_
    # the second restart, reproduced: the generator's second draw as a fixed start
    probe = E.EcgTokenizer(k=8)
    st = probe._record_store(x, None, None)
    rng = np.random.default_rng(7)
    first = probe._random_init(st, 37, rng).cpu().numpy()
    second = probe._random_init(st, 37, rng).cpu().numpy()
    assert len(np.unique(first, axis=0)) == 37 and np.abs(first.mean(axis=1)).max() < 1e-6
    f1 = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(n_clusters=37, init=first, max_iter=8))
    f2 = E.EcgTokenizer(k=8).fit(x, cls_kwargs=dict(n_clusters=37, init=second, max_iter=8))
    print('inertia of the two restarts:', f1.inertia_, f2.inertia_)
    assert one.inertia_ == f1.inertia_ and np.array_equal(one.centers, f1.centers)
    assert two.inertia_ == min(f1.inertia_, f2.inertia_)
    assert np.array_equal(two.centers, (f1 if f1.inertia_ <= f2.inertia_ else f2).centers)
    assert int(two.lens.sum()) == 4 * 12 * 26


# ---- 6. the fixture through the public class -----------------------------------------------------------
def test_fixture_parity():
    z = np.load(os.path.join(GOLDEN, 'tokenizer.npz'))
    th = int(z['th'])
    off_fixture = n_segments = 0
    for i, (k, V, mode, L) in enumerate(json.loads(bytes(z['cases']).decode())):
        sig, centers, lens = z[f'case{i}_sig'], z[f'case{i}_centers'], z[f'case{i}_lens']
        tok = E.EcgTokenizer.from_centers(centers, lens, pad=mode)
        x = torch.from_numpy(sig).to(DEV)
        before = x.clone()
        T = L // k + 1
        for tag, t, table in (('', None, centers), ('_th', th, centers[lens >= th])):
            ids, means = tok(x, th=t)
            assert ids.shape == means.shape == (3, 12, T) and ids.dtype == torch.int32 and means.dtype == torch.float32
            assert torch.equal(x, before)                              # the caller's signal is not modified
            h_ids, h_means = ids.cpu().numpy(), means.cpu().numpy()
            assert h_ids.max() < len(table)                            # with th the ids index the cut table
            share = check_choice(sig, k, mode, table, h_ids, h_means, ids_best=z[f'case{i}_ids{tag}'].reshape(-1), label=f'case {i}{tag}')
            off_fixture += int(round(share * h_ids.size))
            n_segments += h_ids.size
            assert np.all(np.abs(h_means - z[f'case{i}_means{tag}']) <= k * U * np.abs(R.pad(sig.astype(np.float64), k, mode)).reshape(3, 12, T, k).mean(-1))
            fix_ids = torch.from_numpy(z[f'case{i}_ids{tag}'][0, :2].astype(np.int32)).to(DEV)
            dec = tok.decode(fix_ids, th=t)
            assert np.array_equal(dec.cpu().numpy().astype(np.float64), z[f'case{i}_dec{tag}'])
            rec = tok.reconstruct(ids, means, L, th=t)
            want = (tok.decode(ids, th=t) + means[..., None]).reshape(3, 12, T * k)[..., :L]
            assert rec.shape == (3, 12, L) and same_bits(rec, want)
        # the same records as a ragged store of unequal lengths: reconstruct is cut to each record's length
        lengths = [L, L - 3, L]
        store = torch.cat([x[0], x[1][:, :L - 3], x[2]], dim=1).contiguous()
        off = np.concatenate([[0], np.cumsum(lengths)])
        if mode == 'shift' and (L - 3) < k - (L - 3) % k:
            continue
        r_ids, r_means, seg_off = tok(store, offsets=off)
        rec = tok.reconstruct(r_ids, r_means, np.array(lengths))
        assert rec.shape == store.shape
        for r, l in enumerate(lengths):
            a, b = int(seg_off[r]), int(seg_off[r + 1])
            want = (tok.decode(r_ids[:, a:b]) + r_means[:, a:b, None]).reshape(12, -1)[:, :l]
            assert same_bits(rec[:, off[r]:off[r] + l], want)
    # the third part of the rule of case 2, against the reference's own ids: at most 1 segment in 1 000 off them.  A case holds 108 or 288
    # segments, where that cap would mean none at all, so the share is pooled over every case and both tables
    print(f'off the fixture ids: {off_fixture} of {n_segments} segments')
    assert n_segments >= 1900 and off_fixture <= 1e-3 * n_segments

