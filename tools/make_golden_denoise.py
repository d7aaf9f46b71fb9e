#!/usr/bin/env python3
"""Generate tests/golden/denoise.npz by EXECUTING THE REFERENCE'S OWN `butterworth_low_pass`, `est_noise_std` and `nlm`
(ecg_transformer/preprocess/data_preprocessor.py:48-58, :76-80, :83-148) and scipy's filter design.

Runs only where the reference checkout is present (as tools/make_golden_tokenizer.py, whose import stubs it shares); the fixture is data only.
Nothing here is read by tests / smoke / bench.  Every case is one record of 12 leads: a synthetic beat train plus Gaussian noise and baseline
sway, drawn as f32 and handed to the reference as f64.

  ord_{f} / b_{f} / a_{f} / zi_{f}        signal.buttord + butter + lfilter_zi at the reference's band edges, f in 500, 250
  lp_{n}_in / _out                         butterworth_low_pass (500 Hz design), n in LP_LENGTHS (13 = padlen + 1);  lp250_64_out: fqs = 250 on lp_64_in
  sg_{n}_in / _out                         est_noise_std per lead, n in SG_LENGTHS
  nlm{i}_in / _sigma / _out                nlm(sig, 1.5, sch_wd, patch_wd) per lead and its est_noise_std, NLM_CASES[i] = (n, p, sch_wd)
  nlmconst_in                              a record whose lead 3 is constant at 0 (sigma exactly 0): input only, the reference returns NaN there.
                                           (A NON-zero constant does not give sigma 0: the in-place recurrence of est_noise_std turns it into a
                                           decaying alternating tail, whose median deviation is tiny but positive.)
usage:  python tools/make_golden_denoise.py <reference checkout>        (from the repository root)"""
import importlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'denoise.npz')
sys.path.insert(0, REPO)

LP_LENGTHS = [13, 14, 64, 257]
SG_LENGTHS = [3, 4, 22, 23, 64, 161, 256]
NLM_CASES = [(21, 10, None), (22, 10, None), (23, 10, None), (64, 3, None), (160, 10, None), (257, 10, None), (257, 10, 40), (300, 5, 1)]


def record(rng, n):
    """12 leads: beats every ~41 samples, noise, sway"""
    t = np.arange(n, dtype=np.float64)
    out = np.empty((12, n), np.float32)
    for c in range(12):
        beats = sum(np.exp(-0.5 * ((t - t0) / 2.5) ** 2) for t0 in np.arange(rng.uniform(0, 41), n + 41, 41))
        sway = 0.2 * np.sin(2 * np.pi * t / rng.uniform(150, 400) + rng.uniform(0, 6))
        out[c] = (rng.uniform(0.5, 1.5) * beats + sway + rng.normal(0, 0.05, n)).astype(np.float32)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from oracle import make_golden
    make_golden._install_stubs()
    sys.path.insert(0, sys.argv[1])
    M = importlib.import_module('ecg_transformer.preprocess.data_preprocessor')
    from scipy import signal
    D = M.DataPreprocessor
    cfg = D.CONFIG['low_pass']
    rng = np.random.default_rng(2301)
    out = dict(nlm_cases=np.frombuffer(json.dumps(NLM_CASES).encode(), np.uint8), lp_lengths=np.array(LP_LENGTHS), sg_lengths=np.array(SG_LENGTHS),
               band=np.array([cfg['passband'], cfg['stopband'], cfg['passband_ripple'], cfg['stopband_attenuation']], np.float64),
               nlm_defaults=np.array([D.CONFIG['nlm']['smooth_factor'], D.CONFIG['nlm']['window_size']], np.float64))
    for f in (500, 250):
        nyq = 0.5 * f
        o, wn = signal.buttord(cfg['passband'] / nyq, cfg['stopband'] / nyq, cfg['passband_ripple'], cfg['stopband_attenuation'])
        b, a = signal.butter(o, wn, btype='low')
        out.update({f'ord_{f}': np.array(o), f'b_{f}': b, f'a_{f}': a, f'zi_{f}': signal.lfilter_zi(b, a)})
    for n in LP_LENGTHS:
        x = record(rng, n)
        out[f'lp_{n}_in'], out[f'lp_{n}_out'] = x, D.butterworth_low_pass(x.astype(np.float64))
    out['lp250_64_out'] = D.butterworth_low_pass(out['lp_64_in'].astype(np.float64), fqs=250)
    for n in SG_LENGTHS:
        x = record(rng, n)
        out[f'sg_{n}_in'], out[f'sg_{n}_out'] = x, np.array([D.est_noise_std(l) for l in x.astype(np.float64)])
    for i, (n, p, sw) in enumerate(NLM_CASES):
        x = record(rng, n)
        x64 = x.astype(np.float64)
        out[f'nlm{i}_in'] = x
        out[f'nlm{i}_sigma'] = np.array([D.est_noise_std(l) for l in x64])
        out[f'nlm{i}_out'] = np.stack([D.nlm(l, scale=1.5, sch_wd=sw, patch_wd=p) for l in x64])
    x = record(rng, 64)
    x[3] = np.float32(0)
    out['nlmconst_in'] = x
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes;', len(out), 'arrays')


if __name__ == '__main__':
    main()
