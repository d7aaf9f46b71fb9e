#!/usr/bin/env python3
"""Generate tests/golden/dynamic_normalize.npz by EXECUTING THE REFERENCE'S OWN `DynamicNormalize` (ecg_transformer/preprocess/transform.py:108-137).

Runs only where the reference checkout is present (as oracle/make_golden.py, whose import stubs it borrows); the fixture is data only: the
inputs, every stage's `norm_meta` and the reference's transformed output of two records.  Nothing here is read by tests / smoke / bench.

Inputs are drawn as f32 and handed to the reference as f64, as h5py hands it f64.  Two stores over 7 records:
  rect    (7, 12, 160) with NaN samples inside two records (the reference's PTB-XL record 12721 has such) and a run of exact zeros
  ragged  (12, S_total) + offsets, record lengths 130, 257, 3, 1, 97, 200, 61.  A ragged corpus has no rectangle: its truth is the reference
          run on the records padded to the longest one with NaN, which the nan-functions ignore
each fitted whole and on the non-contiguous subset `idxs`, under every scheme of SCHEMES.
usage:  python tools/make_golden_normalize.py <reference checkout>        (from the repository root)"""
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'dynamic_normalize.npz')
sys.path.insert(0, REPO)

SCHEMES = ['global', 'std', ('std', 3), 'norm', ('norm', 3), [('norm', 3), ('std', 1)], 'none']
LENGTHS = [130, 257, 3, 1, 97, 200, 61]
IDXS = [0, 1, 4, 6]
CHAIN = 5          # SCHEMES[CHAIN]: the default chain, whose transformed output of records 0 and 1 is kept


def metas(dn):
    out = np.full((len(dn.normalizers), 2, 12), np.nan, np.float32)
    for j, nz in enumerate(dn.normalizers):
        if nz.norm_meta is not None:
            a, b = nz.norm_meta
            assert a.dtype == np.float32 and a.shape == (1, 12, 1)
            out[j, 0], out[j, 1] = a.reshape(12), b.reshape(12)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    from oracle import make_golden
    make_golden._install_stubs()
    sys.path.insert(0, ref)
    T = importlib.import_module('ecg_transformer.preprocess.transform')
    rng = np.random.default_rng(1812)
    scale = np.linspace(0.05, 0.4, 12)[None, :, None]
    shift = np.linspace(-0.3, 0.2, 12)[None, :, None]
    rect = (rng.standard_normal((len(LENGTHS), 12, 160)) * scale + shift).astype(np.float32)
    rect[2, :, 40:47] = np.nan
    rect[5, 3, 100:] = np.nan
    rect[4, :, :25] = 0.0
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    ragged = (rng.standard_normal((12, int(off[-1]))) * scale[0] + shift[0]).astype(np.float32)
    ragged[:, off[1] + 11:off[1] + 14] = np.nan
    ragged[7, off[5]:off[5] + 30] = 0.0
    padded = np.full((len(LENGTHS), 12, max(LENGTHS)), np.nan, np.float64)
    for i, l in enumerate(LENGTHS):
        padded[i, :, :l] = ragged[:, off[i]:off[i] + l]
    out = dict(rect=rect, ragged=ragged, offsets=off, idxs=np.array(IDXS, np.int64), schemes=np.frombuffer(json.dumps(SCHEMES).encode(), np.uint8))
    for store, sig in (('rect', rect.astype(np.float64)), ('ragged', padded)):
        for tag, arr in (('all', sig), ('idxs', sig[IDXS])):
            for k, scheme in enumerate(SCHEMES):
                norm = scheme if isinstance(scheme, str) else (tuple(scheme) if not isinstance(scheme[0], list) else [tuple(s) for s in scheme])
                dn = T.DynamicNormalize(arr, normalize=norm)
                out[f'{store}_{tag}_{k}_meta'] = metas(dn)
                if k == CHAIN and tag == 'all':
                    out[f'{store}_out'] = np.stack([dn(sig[0]), dn(sig[1])])          # f64, (2, 12, L); NaN where the input is NaN / padding
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
