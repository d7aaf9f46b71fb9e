"""GPU: the DBSCAN kernels (csrc/dbscan.hip) and their route through `EcgTokenizer` against the numpy restatement (tests/dbscan_ref.py), which
tests/test_dbscan.py holds to sklearn itself.  Labels and core sets are compared for equality, with no tolerance: on the exact-integer tables
every f32 operation of the distance is exact, and on general data the test first asserts that no pair lies within 2e-5 of eps (ten times the
f32 chain's bound at k = 32), so both decide every pair alike.

Sizes.  Every table stays under about 6 000 segments.  The edge cases are built from the kernels' own constants: DBSCAN_TILE segments per LDS
tile of the column side, DBSCAN_ROWS[k] rows per workgroup, and DBSCAN_PAIRS_PER_LAUNCH patched down so that a sweep is several launches.

The tables of the edge cases lie on a line: point t is t * u with u = +1 +1 -1 -1 on four samples, |u| = 2 = eps, so t's neighbours are
t - 1, t, t + 1 and a pair of neighbours lies at exactly eps."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import tokenizer
from ecg_representation_learning_amd.tokenizer import DBSCAN_TILE, DBSCAN_ROWS
import dbscan_ref as D

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TILE = DBSCAN_TILE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def on_table(tok, segs, eps, ms):
    """the passes over a dense table -> (core, labels, roots) as numpy arrays"""
    core, labels, roots = tok._dbscan(torch.from_numpy(np.ascontiguousarray(segs, np.float32)).to(DEV), tokenizer.check_eps(eps), ms)
    torch.cuda.synchronize()
    return core.cpu().numpy(), labels.cpu().numpy().astype(np.int64), None if roots is None else roots.cpu().numpy()


def assert_equals_restatement(got_core, got_labels, segs, eps, ms, what=''):
    r = D.run(segs, eps, ms)
    print(f'{what}: n = {len(segs)}, {len(r["core"])} core, {r["clusters"]} clusters, {r["noise"]} noise, {r["ties"]} pairs at eps, {r["contested"]} contested; '
          f'core equal {np.array_equal(got_core, r["core"])}, labels equal {np.array_equal(got_labels, r["labels"])}')
    assert got_core.dtype == np.int64 and got_labels.dtype == np.int64
    assert np.array_equal(got_core, r['core']) and np.array_equal(got_labels, r['labels'])
    return r


def line(ts, k, seed=0):
    """(len(ts), k) f32: t * u, in a shuffled order"""
    u = np.zeros(k, np.float32)
    u[[0, 1]], u[[2, 3]] = 1, -1
    ts = np.random.default_rng(seed).permutation(np.asarray(ts, np.float32))
    return ts[:, None] * u[None, :]


# ---- 1. exact-integer stores --------------------------------------------------------------------------------
@pytest.mark.parametrize('k,mode', [(8, 'zero'), (8, 'shift'), (16, 'zero'), (16, 'shift'), (32, 'zero'), (32, 'shift')])
def test_exact_integer_stores_equal_the_restatement_and_sklearn(k, mode):
    """the stores of tests/test_dbscan.py with this k and padding, one by one as rectangles, then all their records as one ragged store (more than
    one workgroup's rows)"""
    cases = [c for c in map(D.integer_case, range(100, 172)) if (c[0], c[1]) == (k, mode)]
    assert len(cases) == 12
    tok = E.EcgTokenizer(k=k, pad=mode)
    several = ties = 0
    for _, _, eps, ms, x in cases:
        segs, _ = D.segments32(x, k, mode)
        core, labels = tok.dbscan(torch.from_numpy(x).to(DEV), eps, ms)
        r = assert_equals_restatement(core, labels, segs, eps, ms, f'k={k} {mode} eps={eps} ms={ms}')
        sk_core, sk_labels = D.sklearn_dbscan(segs, eps, ms)
        assert np.array_equal(core, sk_core) and np.array_equal(labels, sk_labels)
        several += r['clusters'] > 1
        ties += r['ties'] > 0
    assert several > 0 and ties > 0
    recs = [rec for c in cases for rec in c[4]]
    off = np.concatenate([[0], np.cumsum([r.shape[1] for r in recs])]).astype(np.int64)
    segs, _ = D.segments32(recs, k, mode)
    assert DBSCAN_ROWS[k] < len(segs) <= 6000
    for eps, ms in ((2.0, 4), (1.5, 3)):
        core, labels = tok.dbscan(torch.from_numpy(np.concatenate(recs, axis=1)).to(DEV), eps, ms, offsets=off)
        assert_equals_restatement(core, labels, segs, eps, ms, f'k={k} {mode} ragged eps={eps} ms={ms}')
        sk_core, sk_labels = D.sklearn_dbscan(segs, eps, ms)
        assert np.array_equal(core, sk_core) and np.array_equal(labels, sk_labels)


# ---- 2. tile edges --------------------------------------------------------------------------------------------
def edge_tables(k):
    """name -> (table, min_samples, core count, non-core count) at eps = 2"""
    rpb = DBSCAN_ROWS[k]
    far = lambda m, start=1000: [start + 3 * i for i in range(m)]                    # m isolated points: nobody's neighbours
    out = {}
    for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, rpb - 1, rpb + 1):
        out[f'noise n={n}'] = (line(far(n), k, n), 2, 0, n)                          # no core point at all
        out[f'chain n={n}'] = (line(range(n), k, n), 1 if n == 1 else 2, n, 0)       # every point core, one cluster
    out['one core, tile + 1 others'] = (line([-1, 0, 1] + far(TILE - 1), k, 1), 3, 1, TILE + 1)
    out['tile + 1 core, one other'] = (line([0] + list(range(TILE + 1)), k, 3), 3, TILE + 1, 1)        # the doubled end is core, the other end is not
    out['tile + 1 core, tile + 1 others'] = (line(list(range(TILE + 3)) + far(TILE - 1), k, 4), 3, TILE + 1, TILE + 1)
    out['two blocks of rows, three clusters'] = (line(list(range(rpb)) + list(range(rpb + 5, 2 * rpb)) + far(7, 3 * rpb) + [3 * rpb + 1, 3 * rpb + 2], k, 5), 3,
                                                 None, None)
    return out


@pytest.mark.parametrize('k', [8, 16, 32])
def test_tile_and_block_edges(k, monkeypatch):
    """n at every edge of the column tile and of a workgroup's rows, the core and the non-core count each 0, 1 and tile + 1; every sweep is
    enqueued as one launch per workgroup of rows"""
    monkeypatch.setattr(tokenizer, 'DBSCAN_PAIRS_PER_LAUNCH', 1)
    tok = E.EcgTokenizer(k=k)
    seen_core, seen_rest = set(), set()
    for name, (table, ms, n_core, n_rest) in edge_tables(k).items():
        assert len(tok._row_blocks(len(table), len(table))) == -(-len(table) // DBSCAN_ROWS[k])
        core, labels, _ = on_table(tok, table, 2.0, ms)
        r = assert_equals_restatement(core, labels, table, 2.0, ms, f'k={k} {name}')
        if n_core is not None:
            assert (len(core), len(table) - len(core)) == (n_core, n_rest), name
        seen_core.add(len(core))
        seen_rest.add(len(table) - len(core))
        assert r['ties'] > 0 or name.startswith('noise') or len(table) == 1
    assert {0, 1, TILE + 1} <= seen_core and {0, 1, TILE + 1} <= seen_rest


# ---- 3. a shuffled chain ------------------------------------------------------------------------------------------
def test_shuffled_chain_is_one_cluster():
    """segments t * u for t = 0 .. 2999 in a permuted order, through the store: one cluster whose diameter is the whole store, its two ends
    border segments.  u ends in zeros, so the zero-padded last sample of every lead leaves the last segment what it is."""
    k, T = 8, 250
    u = np.array([1, 1, -1, -1, 0, 0, 0, 0], np.float32)
    t = np.random.default_rng(9).permutation(12 * T).astype(np.float32)
    x = (t[:, None] * u[None, :]).reshape(1, 12, T * k)[..., :T * k - 1].copy()
    tok = E.EcgTokenizer(k=k, pad='zero')
    segs, _ = D.segments32(x, k, 'zero')
    assert segs.shape == (12 * T, k) and np.array_equal(segs, t[:, None] * u[None, :])
    core, labels = tok.dbscan(torch.from_numpy(x).to(DEV), 2.0, 3)
    ends = np.sort(np.concatenate([np.flatnonzero(t == 0), np.flatnonzero(t == 12 * T - 1)]))
    assert np.array_equal(labels, np.zeros(12 * T, np.int64))
    assert np.array_equal(core, np.setdiff1d(np.arange(12 * T), ends))
    assert_equals_restatement(core, labels, segs, 2.0, 3, 'shuffled chain')


# ---- 4. duplicates and degenerate stores ------------------------------------------------------------------------------
def test_duplicates_and_degenerate_stores():
    k = 8
    tok = E.EcgTokenizer(k=k, pad='zero')
    rng = np.random.default_rng(21)
    # many bit-equal segments: 12 x 40 segments drawn from five distinct ones, d = 0 inside a group
    motifs = rng.integers(-2, 3, (5, k)).astype(np.float32)
    x = motifs[rng.integers(0, 5, (1, 12, 40))].reshape(1, 12, 40 * k)[..., :40 * k - 3].copy()
    segs, _ = D.segments32(x, k, 'zero')
    core, labels = tok.dbscan(torch.from_numpy(x).to(DEV), 0.5, 4)
    r = assert_equals_restatement(core, labels, segs, 0.5, 4, 'duplicates')
    assert r['clusters'] >= 3
    # all noise: distinct segments, a tiny eps, min_samples = 2
    y = np.cumsum(rng.standard_normal((1, 12, 203)), axis=-1).astype(np.float32)
    core, labels = tok.dbscan(torch.from_numpy(y).to(DEV), 1e-6, 2)
    assert len(core) == 0 and core.dtype == np.int64 and np.array_equal(labels, np.full(12 * 26, -1, np.int64))
    with pytest.raises(ValueError, match=r'eps.*312'):
        tok.fit(torch.from_numpy(y).to(DEV), method=E.Dbscan(min_samples=2), cls_kwargs=dict(eps=1e-6))
    # all one cluster: an eps beyond every distance
    core, labels = tok.dbscan(torch.from_numpy(y).to(DEV), 1e4, 5)
    assert np.array_equal(core, np.arange(312)) and np.array_equal(labels, np.zeros(312, np.int64))
    # one non-finite sample: its segment is noise, the rest is as without it
    z = D.random_walk_store(1, k)
    segs, _ = D.segments32(z, k, 'zero')
    for bad in (np.nan, np.inf):
        zz = z.copy()
        zz.reshape(-1, 150)[3, 2 * k + 1] = bad                                      # lead 3 of record 0, segment 2: flat segment 3 * 19 + 2 = 59
        q = 3 * 19 + 2
        core, labels = tok.dbscan(torch.from_numpy(zz).to(DEV), 0.06, 5)
        assert labels[q] == -1 and q not in core
        assert np.array_equal(np.delete(labels, q), D.dbscan(np.delete(segs, q, axis=0), 0.06, 5)[1])


# ---- 5. store forms ---------------------------------------------------------------------------------------------------
def test_store_forms_and_segments():
    """a rectangle, the same records ragged, a scrambled subset, a view at an odd offset of a larger buffer: `segments` is bit-equal to the
    restatement in each, and the labels are those of the restatement of the selected records"""
    k, eps, ms = 8, 0.06, 5
    tok = E.EcgTokenizer(k=k, pad='shift')
    n, L = 5, 150
    rect = D.random_walk_store(3, k, (n, 12, L))
    x = torch.from_numpy(rect).to(DEV)
    ragged = torch.from_numpy(np.ascontiguousarray(rect.transpose(1, 0, 2)).reshape(12, n * L)).to(DEV)
    off = np.arange(n + 1) * L

    def check(store, offsets, idxs, recs):
        want_s, want_m = D.segments32(recs, k, 'shift')
        segs, means = tok.segments(store, offsets=offsets, idxs=idxs)
        assert segs.is_cuda and means.is_cuda and segs.dtype == means.dtype == torch.float32 and segs.shape == want_s.shape and means.shape == want_m.shape
        assert np.array_equal(bits(segs.cpu().numpy()), bits(want_s)) and np.array_equal(bits(means.cpu().numpy()), bits(want_m))
        core, labels = tok.dbscan(store, eps, ms, offsets=offsets, idxs=idxs)
        r = assert_equals_restatement(core, labels, want_s, eps, ms, f'offsets={offsets is not None} idxs={idxs}')
        assert r['band'] > 2e-5
        return core, labels

    a = check(x, None, None, rect)
    b = check(ragged, off, None, rect)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    sel = [3, 0, 4]
    c = check(x, None, sel, rect[sel])
    d = check(ragged, off, np.array(sel), rect[sel])
    assert np.array_equal(c[1], d[1])
    buf = torch.zeros(12 * n * L + 4, dtype=torch.float32, device=DEV)               # the store's first sample one float past a 16-byte boundary
    view = buf[1:1 + 12 * n * L].view(12, n * L)
    view.copy_(ragged)
    assert view.data_ptr() % 16 == 4
    e = check(view, off, None, rect)
    assert np.array_equal(e[1], a[1])
    with pytest.raises(ValueError, match='contiguous'):
        tok.dbscan(x[:, :, ::2], eps, ms)
    # records of unequal lengths, one of them a multiple of k (a whole padded segment) and one shorter than a segment
    lengths = [61, 8, 16, 257, 5]
    recs = [np.cumsum(np.random.default_rng(30 + i).standard_normal((12, l)) * 0.05, axis=-1).astype(np.float32) for i, l in enumerate(lengths)]
    roff = np.concatenate([[0], np.cumsum(lengths)])
    flat = torch.from_numpy(np.concatenate(recs, axis=1)).to(DEV)
    check(flat, roff, None, recs)
    check(flat, roff, [4, 1, 3], [recs[4], recs[1], recs[3]])


# ---- 6. general data ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k,mode', [(8, 'zero'), (8, 'shift'), (16, 'zero'), (16, 'shift'), (32, 'zero'), (32, 'shift')])
def test_random_walk_stores_equal_the_restatement_and_sklearn(k, mode):
    eps = {8: 0.06, 16: 0.14, 32: 0.35}[k]
    x = D.random_walk_store(1, k)
    segs, _ = D.segments32(x, k, mode)
    core, labels = E.EcgTokenizer(k=k, pad=mode).dbscan(torch.from_numpy(x).to(DEV), eps, 5)
    r = assert_equals_restatement(core, labels, segs, eps, 5, f'k={k} {mode}')
    assert r['band'] > 2e-5 and r['clusters'] >= 2 and r['noise'] > 0
    sk_core, sk_labels = D.sklearn_dbscan(segs, eps, 5)
    assert np.array_equal(core, sk_core) and np.array_equal(labels, sk_labels)


# ---- 7. fit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ragged', [False, True])
def test_fit_builds_the_vocabulary(ragged, monkeypatch):
    k, eps = 8, 0.06
    n, L = 2, 150
    rect = D.random_walk_store(1, k)
    x = torch.from_numpy(rect).to(DEV)
    if ragged:
        store, kw = torch.from_numpy(np.ascontiguousarray(rect.transpose(1, 0, 2)).reshape(12, n * L)).to(DEV), dict(offsets=np.arange(n + 1) * L)
    else:
        store, kw = x, {}
    segs, _ = D.segments32(rect, k, 'shift')
    r = D.run(segs, eps, 4)
    V = r['clusters']
    assert V >= 2 and r['noise'] > 0 and r['band'] > 2e-5
    tok = E.EcgTokenizer(k=k, pad='shift')
    assert tok.fit(store, method=E.Dbscan(min_samples=7), cls_kwargs=dict(eps=eps, min_samples=4), **kw) is tok       # cls_kwargs overrides the object
    labels = r['labels']
    assert tok.fit_method == 'dbscan' and tok.cls_th == eps and tok.n_sig == n and tok.n_noise == r['noise']
    assert tok.centers.shape == (V, k) and tok.centers.dtype == np.float32 and tok.lens.dtype == np.int64
    assert np.array_equal(tok.lens, np.bincount(labels[labels >= 0], minlength=V)) and int(tok.lens.sum()) + tok.n_noise == len(segs)
    s64 = segs.astype(np.float64)
    for j in range(V):                                                              # the update's bound: max_e |c32 - c64| <= 1e-6 max_e |c64| per centre
        c64 = s64[labels == j].mean(axis=0)
        assert np.abs(tok.centers[j] - c64).max() <= 1e-6 * np.abs(c64).max(), j
    # labels_ has the shape and the layout of the ids tok(sig) returns
    T = L // k + 1
    assert tok.labels_.is_cuda and tok.labels_.dtype == torch.int32
    got = tok.labels_.cpu().numpy()
    if ragged:
        assert got.shape == (12, n * T)
        got = got.reshape(12, n, T).transpose(1, 0, 2)
    assert got.shape == (n, 12, T) and np.array_equal(got.reshape(-1), labels)
    # the new table serves the unchanged encode / decode / reconstruct / th
    ids, means = tok(x)
    assert ids.shape == (n, 12, T) and int(ids.min()) >= 0 and int(ids.max()) < V
    d = ((s64[:, None, :] - tok.centers[None].astype(np.float64)) ** 2).sum(-1)
    flat = ids.cpu().numpy().reshape(-1)
    assert np.all(d[np.arange(len(segs)), flat] - d.min(axis=1) <= 1e-5 * (1 + d.min(axis=1)))
    assert np.array_equal(tok.decode(ids).cpu().numpy(), tok.centers[ids.cpu().numpy()])
    assert tok.reconstruct(ids, means, L).shape == (n, 12, L)
    th = int(tok.lens.max())                                                         # keeps the largest cluster(s) only
    kept = tok.lens >= th
    assert 1 <= kept.sum() < V
    ids_th, _ = tok(x, th=th)
    assert int(ids_th.max()) < int(kept.sum()) and np.array_equal(tok._rows(th), tok.centers[kept])
    # too many clusters for a vocabulary: fit refuses with the count, dbscan() still returns the labels
    monkeypatch.setattr(tokenizer, 'MAX_CLUSTERS', V - 1)
    with pytest.raises(ValueError, match=str(V)):
        E.EcgTokenizer(k=k, pad='shift').fit(store, method=E.Dbscan(min_samples=4), cls_kwargs=dict(eps=eps), **kw)
    assert np.array_equal(tok.dbscan(store, eps, 4, **kw)[1], labels)
    monkeypatch.undo()
    # a k-means fit afterwards still works, and drops what belonged to the DBSCAN table
    tok.fit(store, method='kmeans', cls_kwargs=dict(n_clusters=6, random_state=0), **kw)
    assert tok.fit_method == 'kmeans' and tok.centers.shape == (6, k) and int(tok.lens.sum()) == len(segs) and tok.cls_th == 6
    assert tok.n_noise is None and tok.labels_ is None


# ---- 8. reproducibility ---------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_roots_and_labels(monkeypatch):
    """twice, not in a loop: the root of a component is its smallest compact index whatever the order the edges arrive in"""
    k = 16
    cases = [c for c in map(D.integer_case, range(100, 172)) if c[0] == k]
    segs = np.concatenate([D.segments32(c[4], k, c[1])[0] for c in cases])
    assert DBSCAN_ROWS[k] < len(segs) <= 6000
    monkeypatch.setattr(tokenizer, 'DBSCAN_PAIRS_PER_LAUNCH', 1)
    tok = E.EcgTokenizer(k=k)
    a, b = on_table(tok, segs, 1.5, 3), on_table(tok, segs, 1.5, 3)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    r = assert_equals_restatement(a[0], a[1], segs, 1.5, 3, 'twice')
    assert r['clusters'] > 1
    roots = a[2]
    assert np.array_equal(np.unique(roots, return_inverse=True)[1], r['labels'][r['core']])
    first = {}                                                                        # a root is the first (smallest) compact index of its cluster
    for i, lab in enumerate(r['labels'][r['core']]):
        first.setdefault(int(lab), i)
    assert np.array_equal(roots, np.array([first[int(lab)] for lab in r['labels'][r['core']]]))
