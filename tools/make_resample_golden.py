#!/usr/bin/env python3
"""Generate tests/golden/resample.npz with scipy: what the reference's export stage computes per lead (preprocess/data_export.py:202-215:
`wfdb.processing.resample_sig(sig, fqs, 250)`, which reduces to `scipy.signal.resample(sig, int(n * 250 / fqs))`).  `wfdb` is not available:
the fixture pins the scipy call, and the length rule is restated in `resample.resampled_length`.  Nothing of the reference is run or read.

  cases                 json [[n_in, n_out], ...]
  r{i}_in               one record, (12, n_in) float32: beats, sway and noise (tests/resample_ref.py `record`)
  r{i}_out64            scipy.signal.resample of the input cast to float64 (float64)
  r{i}_out32            scipy.signal.resample of the float32 input: exactly the reference's call, which scipy runs in single precision (float32)
usage:  python tools/make_resample_golden.py        (from the repository root; needs scipy)"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'resample.npz')
sys.path.insert(0, os.path.join(REPO, 'tests'))

CASES = [(257, 250), (96, 60), (40, 64), (31, 17)]     # 257 Hz -> 250 Hz on a second of INCART; N even down, N even up, N odd


def main():
    from scipy import signal
    from resample_ref import record
    rng = np.random.default_rng(2310)
    out = dict(cases=np.frombuffer(json.dumps(CASES).encode(), np.uint8))
    for i, (n, num) in enumerate(CASES):
        x = record(rng, n)
        y32 = signal.resample(x, num, axis=-1)
        assert y32.dtype == np.float32
        out[f'r{i}_in'], out[f'r{i}_out64'], out[f'r{i}_out32'] = x, signal.resample(x.astype(np.float64), num, axis=-1), y32
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
