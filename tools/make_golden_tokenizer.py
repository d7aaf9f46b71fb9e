#!/usr/bin/env python3
"""Generate tests/golden/tokenizer.npz by EXECUTING THE REFERENCE'S OWN `EcgPadder` and `EcgTokenizer.__call__` / `decode`
(ecg_transformer/models/ecg_tokenizer.py:88-137, :222-258, :346-350).

Runs only where the reference checkout is present (as tools/make_golden_normalize.py, whose import stubs it shares); the fixture is data only.
Nothing here is read by tests / smoke / bench.

The reference's tokenizer is given a vocabulary instead of being fitted: `centers`, `lens` and a `KDTree` over the centres are set on the
object, which is all `__call__` and `decode` read.  Its module names `ic` outside `__main__` and its `th` path logs through `log` / `logi`,
which the shared stubs do not cover: no-ops are set in the module.  Inputs are drawn as f32 and handed to the reference as f64.

  pad_{mode}_{l}_in / _out      EcgPadder(k=8, mode) on a (2, l) array, l in 9, 13, 16, 61
  case{i}_sig / _centers / _lens, case{i}_ids / _means / _dec, case{i}_ids_th / _means_th / _dec_th   (th = 10), for CASES[i] = (k, V, pad, L)
usage:  python tools/make_golden_tokenizer.py <reference checkout>        (from the repository root)"""
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'tokenizer.npz')
sys.path.insert(0, REPO)

PAD_LENGTHS = [9, 13, 16, 61]
CASES = [(8, 37, 'shift', 61), (8, 300, 'zero', 64), (16, 100, 'shift', 61), (32, 64, 'zero', 64), (8, 64, 'shift', 16)]   # (k, V, pad, L)
TH = 10


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    from oracle import make_golden
    make_golden._install_stubs()
    sys.path.insert(0, ref)
    M = importlib.import_module('ecg_transformer.models.ecg_tokenizer')
    M.ic = lambda *a, **k: None
    M.log = lambda *a, **k: None
    M.logi = lambda *a, **k: ''
    from sklearn.neighbors import KDTree
    rng = np.random.default_rng(2204)
    out = dict(cases=np.frombuffer(json.dumps(CASES).encode(), np.uint8), pad_lengths=np.array(PAD_LENGTHS), th=np.array(TH))
    for mode in ('zero', 'shift'):
        for l in PAD_LENGTHS:
            x = rng.normal(0.3, 0.7, (2, l)).astype(np.float32)
            out[f'pad_{mode}_{l}_in'] = x
            out[f'pad_{mode}_{l}_out'] = M.EcgPadder(8, mode)(x.astype(np.float64))
    for i, (k, V, mode, L) in enumerate(CASES):
        sig = rng.normal(0.3, 0.7, (3, 12, L)).astype(np.float32)
        centers = rng.standard_normal((V, k))
        centers = (centers - centers.mean(axis=1, keepdims=True)).astype(np.float32)
        lens = rng.integers(0, 41, V).astype(np.int64)
        tok = M.EcgTokenizer(k=k, pad=mode)
        tok.centers, tok.lens = centers.astype(np.float64), lens
        tok.nn = KDTree(tok.centers)
        ids, means = tok(sig.astype(np.float64))
        ids_th, means_th = tok(sig.astype(np.float64), th=TH)
        out.update({f'case{i}_sig': sig, f'case{i}_centers': centers, f'case{i}_lens': lens,
                    f'case{i}_ids': ids.astype(np.int64), f'case{i}_means': means, f'case{i}_dec': tok.decode(ids[0, :2]),
                    f'case{i}_ids_th': ids_th.astype(np.int64), f'case{i}_means_th': means_th, f'case{i}_dec_th': tok.decode(ids_th[0, :2], th=TH)})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
