"""Shared by tests/test_normalize_fit.py (CPU) and tests/test_gpu_normalize_fit.py: the fixture tests/golden/dynamic_normalize.npz (written by
tools/make_golden_normalize.py from the reference's own DynamicNormalize) and numpy restatements of the raw per-lead statistics."""
import json
import os

import numpy as np

from conftest import GOLDEN
from ecg_representation_learning_amd import transform as T

_Z = None


def fixture():
    global _Z
    if _Z is None:
        z = np.load(os.path.join(GOLDEN, 'dynamic_normalize.npz'))
        _Z = {k: z[k] for k in z.files}
        _Z['schemes'] = [as_norm_arg(s) for s in json.loads(bytes(_Z['schemes']).decode())]
    return _Z


def as_norm_arg(s):
    """JSON turned the tuples into lists: back to what the reference accepts"""
    if isinstance(s, str):
        return s
    return [tuple(e) for e in s] if isinstance(s[0], list) else tuple(s)


def key(v):
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ulps(a, b):
    """distance in f32 representable values"""
    return np.abs(key(a).astype(np.int64) - key(b).astype(np.int64))


def lead_samples(store, offsets=None, idxs=None):
    """per lead the selected samples, NaN included, as one f32 vector each"""
    store = np.asarray(store)
    if store.ndim == 3:
        sel = store if idxs is None else store[np.asarray(idxs)]
        return [np.ascontiguousarray(sel[:, c, :]).reshape(-1).astype(np.float32) for c in range(store.shape[1])]
    ids = range(len(offsets) - 1) if idxs is None else idxs
    return [np.concatenate([store[c, offsets[i]:offsets[i + 1]] for i in ids]).astype(np.float32) for c in range(store.shape[0])]


def sorted_valid(v):
    """the non-NaN samples in key order (-0.0 below +0.0): as values exactly np.sort"""
    v = v[~np.isnan(v)]
    s = v[np.argsort(key(v), kind='stable')]
    assert np.array_equal(s, np.sort(v))
    return s


def numpy_raw(leads, specs, want_std=True):
    """RawStats by numpy in f64 (np.mean / np.std on the valid samples; percentiles by T.percentile_targets / T.lerp on np.sort)"""
    C = len(leads)
    srt = [sorted_valid(v).astype(np.float64) for v in leads]
    count = np.array([len(s) for s in srt], np.int64)
    raw = T.RawStats(count, np.array([int(np.isnan(v).sum()) for v in leads], np.int64), mean=np.array([s.mean() for s in srt]),
                     std=np.array([s.std() for s in srt]) if want_std else None)
    for spec in specs:
        if spec == 'min':
            raw.order[spec] = np.array([s[0] for s in srt])
        elif spec == 'max':
            raw.order[spec] = np.array([s[-1] for s in srt])
        else:
            o = []
            for s in srt:
                lo, hi, g = T.percentile_targets(spec[1], len(s))
                o.append(T.lerp(s[lo], s[hi], g))
            raw.order[spec] = np.array(o)
    return raw


def check_metas(stages, want, what):
    """every stage's norm_meta against the fixture's (nstage, 2, 12) f32 block (NaN rows: 'none'), within 1 f32 ulp"""
    assert len(stages) == len(want), what
    for j, st in enumerate(stages):
        if st.norm_meta is None:
            assert st.scheme == 'none' and np.isnan(want[j]).all(), what
            continue
        for h in (0, 1):
            assert st.norm_meta[h].dtype == np.float32 and st.norm_meta[h].shape == (12,)
            d = ulps(st.norm_meta[h], want[j, h])
            assert d.max() <= 1, (what, j, h, d, st.norm_meta[h], want[j, h])
