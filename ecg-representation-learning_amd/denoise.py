"""
The reference's Zheng et al. denoiser (`ecg_transformer/preprocess/data_preprocessor.py:22-148`, MATLAB twin `preprocess_matlab/DataPreprocessor.m`
and `nlm.m`) on the device: zero-phase Butterworth low-pass, the robust LOESS baseline it subtracts, the noise estimate and non-local means,
the stage that writes the `*-denoised.hdf5` files every reference run trains on.  The sweeps are HIP kernels (`csrc/denoise.hip`) over the record stores of `records.py`, which
`fit_dynamic_normalize` and `EcgTokenizer` take too: (n, 12, L) float32 records, a ragged (12, S_total) store with `offsets`, a subset `idxs` of either.  A device store is
processed where it lies -- in place with `out=records`, into `out=`, or (default) into a new tensor that starts as a copy, so records outside
`idxs` carry over; a host array / memmap streams through the device `chunk_records` records at a time and comes back as a float32 numpy array.
There is no CPU fallback.

The robust LOESS baseline (`rloess`; `EcgDenoiser()(records, baseline='rloess')` is the whole of the reference's `zheng`) follows the algorithm
of the `loess` package the reference imports, as include/ecgvit_hip.h states it in full.  The package is not available, so parity with the
reference is UNPINNED there: the tests hold the kernel to a numpy f64 restatement.  Two results the reference leaves open are defined here: the
tie of an even window goes to the lower index, and a window whose median absolute residual is 0 keeps the fit it has.

Records longer than `MAX_LEN` = 32768 samples (Holter length; INCART's 30 minutes at 257 Hz are 462 600) run with `tiled=True`, up to
`MAX_LEN_TILED` = 1 << 25 samples: the low-pass and the noise estimate are the same kernels under a higher cap (`ecgvit_filtfilt_long`,
`ecgvit_nlm_sigma_long`: the same bits), the non-local means and the robust LOESS are tiled along time (`ecgvit_nlm_denoise_tiled`,
`ecgvit_rloess_tiled`: grid (record, lead, tile), bit-identical to the resident kernels up to 32768 samples for every tile).  `tile` is the
number of output samples a workgroup owns (None: 7680 for the non-local means, 2048 for the LOESS).  `tiled=True` always runs the new entry
points, on short records too; the default `tiled=False` changes nothing and keeps refusing 32769 samples: nothing dispatches between the two.
A tiled workgroup reads samples that another one writes, so the tiled kernels refuse out == x.  In-place operation (`out=records`, a host
store's staging buffer, the later stages of `EcgDenoiser`) is kept on the host side: each launch group (records worth at most `_WS_BYTES` of
f32) is gathered into a compact scratch, denoised into a second one and scattered back -- two f32 copies of the group (8 bytes per sample and
lead) and an int64 column index (8 bytes per sample) of device memory, and one extra read and write of the group.  Pass a separate `out=` (or
none) to avoid it.
Not built: MATLAB's `smooth(..., 'rloess')` of the twin (another algorithm), NaN samples, non-uniform abscissae, LOESS windows over 1024 samples,
a parallel form of the low-pass recurrence, and any automatic choice between the resident and the tiled kernels.
"""
import ctypes
import math

import numpy as np
import torch

from . import hip
from .hip import lib, run, ptr, stream
from .records import DeviceTables, RecordSelection, check_device_store, host_chunks, select_records

MAX_LEN = hip.DENOISE_MAX_LEN                # samples per record: the resident non-local means and LOESS keep a lead in LDS
MAX_LEN_TILED = hip.DENOISE_MAX_LEN_TILED    # samples per record with tiled=True (24 hours at 360 Hz)
MAX_TAPS = hip.DENOISE_MAX_TAPS
MAX_POINTS = hip.DENOISE_MAX_POINTS          # samples per LOESS window: covers every sampling rate of the reference's config (250, 257, 500, 1000)
MAX_ROBUST_ITERS = hip.DENOISE_MAX_ROBUST_ITERS
NLM_RUN = hip.DENOISE_NLM_RUN                # output samples per run of the non-local means: `tile` is a multiple of it there
NLM_TILE = hip.DENOISE_NLM_MAX_THREADS * NLM_RUN   # the default tile of the non-local means: one run per lane of the widest workgroup
LOESS_LDS = hip.DENOISE_LOESS_LDS            # samples the tiled LOESS keeps in LDS: a tile and two windows
LOESS_TILE = LOESS_LDS - 2 * MAX_POINTS      # its default tile
_MAX_TILES = hip.DENOISE_MAX_TILES           # tiles per lead (the grid's third dimension)
C = 12                     # leads per record: what `select_records` admits
_WS_BYTES = 256 * 2 ** 20  # f64 intermediates of the low-pass / noise estimate per launch: more records go in several launches


# ---- filter design (scipy.signal.buttord / butter / lfilter_zi restated in numpy f64; the product imports no scipy) -----------------
def design_lowpass(fqs=500, passband=50, stopband=60, passband_ripple=1, stopband_attenuation=2.5):
    """-> (b, a, zi): the digital Butterworth low-pass of minimal order that loses at most `passband_ripple` dB up to `passband` Hz and at least
    `stopband_attenuation` dB from `stopband` Hz (`signal.buttord`, `signal.butter(ord, wn, 'low')`), and its `signal.lfilter_zi`.  The defaults
    are the reference's `util/config.py:88-100`; at 500 and 250 Hz the order is 3."""
    nyq = 0.5 * fqs
    wp, ws = passband / nyq, stopband / nyq
    if not (0 < wp < ws < 1):
        raise ValueError(f'a low-pass needs 0 < passband < stopband < fqs / 2, got {passband}, {stopband} at fqs = {fqs}')
    if not (0 < passband_ripple < stopband_attenuation):
        raise ValueError('a low-pass needs 0 < passband_ripple < stopband_attenuation (dB)')
    passb, stopb = math.tan(math.pi * wp / 2.0), math.tan(math.pi * ws / 2.0)       # buttord: pre-warped band edges
    g_stop, g_pass = 10 ** (0.1 * abs(stopband_attenuation)), 10 ** (0.1 * abs(passband_ripple))
    order = int(math.ceil(math.log10((g_stop - 1.0) / (g_pass - 1.0)) / (2 * math.log10(stopb / passb))))
    if not 1 <= order <= MAX_TAPS - 1:
        raise ValueError(f'the design needs order {order}: 1 to {MAX_TAPS - 1} are supported')
    w0 = (g_pass - 1.0) ** (-1.0 / (2.0 * order))
    wn = (2.0 / math.pi) * math.atan(w0 * passb)
    # butter: analogue prototype poles, low-pass to the warped frequency, bilinear transform at fs = 2
    p = -np.exp(1j * math.pi * np.arange(-order + 1, order, 2) / (2 * order))
    warped = 4.0 * math.tan(math.pi * wn / 2.0)
    p = warped * p
    k = warped ** order
    pz = (4.0 + p) / (4.0 - p)
    kz = k * np.real(1.0 / np.prod(4.0 - p))
    b = kz * np.poly(-np.ones(order))
    a = np.real(np.poly(pz))
    b, a = np.ascontiguousarray(b, np.float64), np.ascontiguousarray(a, np.float64)
    return b, a, lfilter_zi(b, a)


def lfilter_zi(b, a):
    """the initial state of the direct-form-II-transposed filter whose step response starts at its final value (`signal.lfilter_zi`)"""
    b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
    if a[0] != 1.0:
        b, a = b / a[0], a / a[0]
    n = max(len(a), len(b))
    a, b = np.r_[a, np.zeros(n - len(a))], np.r_[b, np.zeros(n - len(b))]
    comp = np.zeros((n - 1, n - 1))
    comp[0] = -a[1:]
    comp[np.arange(1, n - 1), np.arange(0, n - 2)] = 1.0
    return np.linalg.solve(np.eye(n - 1) - comp.T, b[1:] - a[1:] * b[0])


def _taps(b, a, zi):
    b, a = np.atleast_1d(np.asarray(b, np.float64)), np.atleast_1d(np.asarray(a, np.float64))
    nt = max(len(a), len(b))
    if b.ndim != 1 or a.ndim != 1 or not 2 <= nt <= MAX_TAPS:
        raise ValueError(f'b and a must be 1-D with 2 to {MAX_TAPS} taps')
    if a[0] != 1.0:
        raise ValueError('a[0] must be 1 (normalise the filter)')
    b, a = np.r_[b, np.zeros(nt - len(b))], np.r_[a, np.zeros(nt - len(a))]
    zi = lfilter_zi(b, a) if zi is None else np.asarray(zi, np.float64)
    if zi.shape != (nt - 1,):
        raise ValueError(f'zi must hold {nt - 1} values')
    if not (np.isfinite(b).all() and np.isfinite(a).all() and np.isfinite(zi).all()):
        raise ValueError('b, a and zi must be finite')
    return np.ascontiguousarray(b), np.ascontiguousarray(a), np.ascontiguousarray(zi), nt


def _dp(arr):
    return arr.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- stores ---------------------------------------------------------------------------------------------------------------------------
_ENTRY = {   # by `tiled`: the entry points that differ only in their cap
    False: dict(workspace='ecgvit_denoise_workspace', filtfilt='ecgvit_filtfilt', sigma='ecgvit_nlm_sigma'),
    True: dict(workspace='ecgvit_denoise_workspace_long', filtfilt='ecgvit_filtfilt_long', sigma='ecgvit_nlm_sigma_long')}


def launches(tab, entry):
    """(first record, records) per launch over the `DeviceTables` tab, so that the f64 workspace of a launch stays within _WS_BYTES"""
    step = max(1, _WS_BYTES // getattr(lib(), entry['workspace'])(1, C, tab.max_len))
    return [(lo, min(step, tab.R - lo)) for lo in range(0, tab.R, step)]


def groups(tab):
    """(first record, records) per launch group of a tiled stage that runs in place: each of the group's two f32 scratch stores stays within
    _WS_BYTES (at 462 600 samples: 12 records)"""
    step = max(1, _WS_BYTES // (4 * C * tab.max_len))
    return [(lo, min(step, tab.R - lo)) for lo in range(0, tab.R, step)]


def compact(tab, lo, cnt):
    """the records lo .. lo + cnt as a compact (12, S) store -> (its offsets as a device table, S, the store column of every compact column)"""
    lens, src = tab.raw_len_h[lo:lo + cnt], tab.src_off_h[lo:lo + cnt]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    S = int(lens.sum())
    cols = np.repeat(src - off, lens) + np.arange(S, dtype=np.int64)
    return torch.from_numpy(off).to(tab.x.device), S, torch.from_numpy(cols).to(tab.x.device)


def _tiled_groups(x, o, tab, launch):
    """Run `launch(x, out, src_off table of the launch's records, lead stride, first record, records)` of a tiled kernel over the records of `tab`.
    Out of place: one launch on the store itself.  In place (the kernels refuse out == x): group by group through two compact scratch stores."""
    if o.data_ptr() != x.data_ptr():
        launch(x, o, tab.src_off, tab.stride, 0, tab.R)
        return
    flat_x, flat_o = x.view(-1), o.view(-1)
    for lo, cnt in groups(tab):
        off, S, cols = compact(tab, lo, cnt)
        a = torch.stack([flat_x[cols + c * tab.stride] for c in range(C)])
        b = a.clone()           # (a lead the kernel leaves alone keeps its samples)
        launch(a, b, off, S, lo, cnt)
        for c in range(C):
            flat_o[cols + c * tab.stride] = b[c]


def _check_tile(tiled, tile, multiple=1):
    """-> the tile in output samples, 0 for the default"""
    if tile is None:
        return 0
    if not tiled:
        raise ValueError(f'tile = {tile!r} needs tiled=True')
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or tile < 1:
        raise ValueError(f'tile = {tile!r}: None or an int, at least 1 (the output samples a workgroup owns)')
    if tile % multiple:
        raise ValueError(f'tile = {tile}: a multiple of {multiple}, the run of the non-local means')
    return int(tile)


def _resolve_out(records, out):
    """out=None: a new tensor that starts as a copy; out is records: in place; else a tensor of the same layout that does not overlap records"""
    if out is None:
        return records.clone()
    if not isinstance(out, torch.Tensor):
        raise ValueError('out must be a device tensor')
    if out is records:
        return out
    check_device_store(out, 'out')
    if out.shape != records.shape or out.device != records.device:
        raise ValueError(f'out must have the shape and device of records, got {tuple(out.shape)} on {out.device}')
    if out.data_ptr() == records.data_ptr():
        return out
    lo, hi = records.data_ptr(), records.data_ptr() + records.numel() * 4
    if out.data_ptr() < hi and lo < out.data_ptr() + out.numel() * 4:
        raise ValueError('out overlaps records without being records: pass out=records to run in place')
    return out


def _resolve(records, offsets, idxs, min_len=1, tiled=False, unique=(True, False)):
    """The one resolution of a public call -> (the store: a device tensor or a host array, its `RecordSelection`), the store and the lengths
    checked.  unique: whether an `idxs` that repeats a record is refused, for (a device store, a host store).  idxs: a `RecordSelection` is
    taken as it is: what `EcgDenoiser` resolved for a store of this layout, `offsets` and repeats included."""
    on_device = isinstance(records, torch.Tensor) and records.is_cuda
    if on_device:
        check_device_store(records)
    else:
        records = records.numpy() if isinstance(records, torch.Tensor) else records
        if not hasattr(records, 'shape') or not hasattr(records, 'dtype') or not np.issubdtype(records.dtype, np.floating):
            raise ValueError('records must be a float32 device tensor or a host array / memmap / tensor of a float type')
    s = idxs if isinstance(idxs, RecordSelection) else select_records(records, offsets, idxs, unique=unique[not on_device])
    if tiled and s.max_len > MAX_LEN_TILED:
        raise ValueError(f'a record of {s.max_len} samples: at most {MAX_LEN_TILED} are supported with tiled=True')
    if not tiled and s.max_len > MAX_LEN:
        raise ValueError(f'a record of {s.max_len} samples: at most {MAX_LEN} are supported (tiled=True takes up to {MAX_LEN_TILED})')
    if s.min_len < min_len:
        raise ValueError(f'a record of {s.min_len} samples: this stage needs at least {min_len}')
    return records, s


def _sweep(records, s, out, chunk_records, stage):
    """Run `stage(x, out, tables, first selected record)` over the records `_resolve` selected.  Device store: one call, returns the output
    tensor.  Host store: chunk by chunk in place on a staging buffer, returns a float32 numpy array (a copy of the input with the selected
    records replaced; `out`, a float32 array of the same shape, is filled instead when given).  out=False: a stage that only reads; it gets
    None for a device store, and nothing comes back from the device for a host one."""
    if isinstance(records, torch.Tensor):
        out = None if out is False else _resolve_out(records, out)
        with torch.cuda.device(records.device):
            stage(records, out, DeviceTables.of(records, s), 0)
        return out
    if out is not None and out is not False:
        if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != records.shape:
            raise ValueError('for a host store, out must be a float32 numpy array of the same shape')
    chunks = host_chunks(records, s, chunk_records)
    if not torch.cuda.is_available():
        raise RuntimeError('the denoiser runs on the device (no CPU fallback exists)')
    if out is None:
        out = np.array(records, dtype=np.float32)
    device = torch.device('cuda')
    first = 0
    with torch.cuda.device(device):
        for buf, off, lens, stride, scatter in chunks:
            x = torch.from_numpy(buf).to(device)
            stage(x, x, DeviceTables(x, off, lens, stride), first)
            if out is not False:
                scatter(out, x.cpu().numpy())
            first += len(lens)
    return out


# ---- the stages -----------------------------------------------------------------------------------------------------------------------
def _workspace(tab, device, entry):
    R = max(cnt for _, cnt in launches(tab, entry))
    return torch.empty(getattr(lib(), entry['workspace'])(R, C, tab.max_len) // 8, dtype=torch.float64, device=device)


def lowpass_taps(records, b, a, zi=None, offsets=None, idxs=None, out=None, chunk_records=None, tiled=False, tile=None):
    """`scipy.signal.filtfilt(b, a, lead)` with its defaults for every lead of the selected records (f64 arithmetic; odd extension by
    3 * max(len(a), len(b)) samples, which every record must exceed).  zi: `lfilter_zi(b, a)` when None.
    tiled: run `ecgvit_filtfilt_long` (the same kernel, records up to `MAX_LEN_TILED` samples, the same bits); `tile` is checked and ignored --
    the recurrence is walked by one lane per lead whatever the length, and runs in place without a scratch."""
    b, a, zi, nt = _taps(b, a, zi)
    _check_tile(tiled, tile)
    entry = _ENTRY[tiled]

    def stage(x, o, tab, first):
        ws = _workspace(tab, x.device, entry)
        for lo, cnt in launches(tab, entry):
            getattr(run, entry['filtfilt'])(ptr(x), ptr(o), ptr(tab.src_off[lo:]), tab.stride, ptr(tab.raw_len[lo:]), cnt, C, tab.min_len,
                                            tab.max_len, _dp(b), _dp(a), _dp(zi), nt, ptr(ws), stream())
    return _sweep(*_resolve(records, offsets, idxs, 3 * nt + 1, tiled), out, chunk_records, stage)


def lowpass(records, fqs=500, passband=50, stopband=60, passband_ripple=1, stopband_attenuation=2.5, offsets=None, idxs=None, out=None,
            chunk_records=None, tiled=False, tile=None):
    """The reference's `butterworth_low_pass` (:48-58): `design_lowpass` then the zero-phase filter.  The reference's `zheng` never passes its
    `fqs` on, so it always filters with the 500 Hz design; the MATLAB twin passes it.  Here `fqs` is explicit.  tiled, tile: `lowpass_taps`."""
    b, a, zi = design_lowpass(fqs, passband, stopband, passband_ripple, stopband_attenuation)
    return lowpass_taps(records, b, a, zi, offsets=offsets, idxs=idxs, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)


def _sigma_of(x, tab, tiled=False):
    """the noise estimate over exactly the records of `tab` (a device store)"""
    entry = _ENTRY[tiled]
    sig = torch.zeros((tab.R, C), dtype=torch.float64, device=x.device)
    ws = _workspace(tab, x.device, entry)
    for lo, cnt in launches(tab, entry):
        getattr(run, entry['sigma'])(ptr(x), ptr(tab.src_off[lo:]), tab.stride, ptr(tab.raw_len[lo:]), cnt, C, tab.max_len, ptr(sig[lo:]),
                                     ptr(ws), stream())
    return sig


def estimate_noise_std(records, offsets=None, idxs=None, chunk_records=None, tiled=False, tile=None):
    """The reference's `est_noise_std` (:76-80) for every lead of the selected records -> (R, 12) float64 device tensor, rows in `idxs` order.
    tiled: run `ecgvit_nlm_sigma_long` (the same kernel, records up to `MAX_LEN_TILED` samples, the same bits); `tile` is checked and ignored."""
    tables = []
    _check_tile(tiled, tile)
    records, s = _resolve(records, offsets, idxs, 1, tiled, unique=(False, False))
    _sweep(records, s, False, chunk_records, lambda x, o, tab, first: tables.append(_sigma_of(x, tab, tiled)))
    return tables[0] if len(tables) == 1 else torch.cat(tables)


def _check_nlm(scale, search_width, patch_width):
    if not (isinstance(patch_width, (int, np.integer)) and patch_width >= 1):
        raise ValueError(f'patch_width = {patch_width!r}: an int, at least 1')
    if search_width is not None and not (isinstance(search_width, (int, np.integer)) and search_width >= 1):
        raise ValueError(f'search_width = {search_width!r}: None (the whole record) or an int, at least 1')
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError(f'scale = {scale!r}: a positive number')


def nlm(records, scale=1.5, search_width=None, patch_width=10, sigma=None, offsets=None, idxs=None, out=None, chunk_records=None, tiled=False,
        tile=None):
    """The reference's `DataPreprocessor.nlm` (:83-148) for every lead of the selected records, quirks included (include/ecgvit_hip.h spells
    them out): f32 arithmetic.  sigma: the (R, 12) float64 table of `estimate_noise_std` over the same selection; None estimates it from
    `records`, as the reference does.  A lead with sigma == 0 (a constant lead) is copied through; the reference returns NaN there.
    The defaults are the reference's (`util/config.py`: smooth_factor 1.5, window_size 10).
    tiled: run `ecgvit_nlm_denoise_tiled` (records up to `MAX_LEN_TILED` samples; the bits of the resident kernel for every record it takes and
    every tile).  tile: the output samples a workgroup owns, a multiple of 15 (None: 7680); a record may need at most 65535 tiles.  In place the
    tiled kernel runs through a scratch (the module's docstring says what it costs)."""
    _check_nlm(scale, search_width, patch_width)
    tile_runs = _check_tile(tiled, tile, NLM_RUN) // NLM_RUN
    tail = (float(scale), int(patch_width), 0 if search_width is None else int(search_width))
    if sigma is not None:
        if isinstance(sigma, np.ndarray):
            sigma = torch.from_numpy(np.ascontiguousarray(sigma, np.float64))
        if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float64 or sigma.dim() != 2 or sigma.shape[1] != 12:
            raise ValueError('sigma must be an (R, 12) float64 table, one row per selected record')

    def stage(x, o, tab, first):
        sig = _sigma_of(x, tab, tiled) if sigma is None else sigma[first:first + tab.R].to(x.device).contiguous()
        if not tiled:
            return run.ecgvit_nlm_denoise(ptr(x), ptr(o), ptr(tab.src_off), tab.stride, ptr(tab.raw_len), tab.R, C, tab.max_len, ptr(sig), *tail,
                                          stream())
        runs = max(1, -(-(tab.max_len - 2 * int(patch_width) - 1) // NLM_RUN))
        if -(-runs // min(tile_runs or NLM_TILE // NLM_RUN, runs)) > _MAX_TILES:
            raise ValueError(f'tile = {tile}: a record of {tab.max_len} samples would need more than {_MAX_TILES} tiles')

        def launch(xs, os_, off, stride, lo, cnt):
            run.ecgvit_nlm_denoise_tiled(ptr(xs), ptr(os_), ptr(off), stride, ptr(tab.raw_len[lo:]), cnt, C, tab.max_len, ptr(sig[lo:]), *tail,
                                         tile_runs, stream())
        _tiled_groups(x, o, tab, launch)
    records, s = _resolve(records, offsets, idxs, 1, tiled)
    if sigma is not None and sigma.shape[0] != s.R:
        raise ValueError(f'sigma holds {sigma.shape[0]} rows for {s.R} selected records')
    return _sweep(records, s, out, chunk_records, stage)


def frac_points(n, frac):
    """the window the reference's `rloess` gives a record of n samples for a float `n`: force_odd(int(sig.size * n) - 1)"""
    return 2 * math.floor((int(n * frac) - 1) / 2) + 1


def _check_rloess_args(npoints, degree, robust_iters):
    """-> (npoints as the kernel takes it, the fraction or 0.0)"""
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or degree not in (1, 2):
        raise ValueError(f'degree = {degree!r}: 1 or 2')
    if isinstance(robust_iters, bool) or not isinstance(robust_iters, (int, np.integer)) or not 0 <= robust_iters <= MAX_ROBUST_ITERS:
        raise ValueError(f'robust_iters = {robust_iters!r}: an int, 0 to {MAX_ROBUST_ITERS}')
    if isinstance(npoints, (float, np.floating)):
        if not 0.0 < npoints < 1.0:
            raise ValueError(f'npoints = {npoints!r}: a fraction lies in (0, 1)')
        return 0, float(npoints)
    if isinstance(npoints, bool) or not isinstance(npoints, (int, np.integer)) or not degree + 2 <= npoints <= MAX_POINTS:
        raise ValueError(f'npoints = {npoints!r}: an int, {degree + 2} (degree + 2) to {MAX_POINTS}, or a fraction in (0, 1)')
    return int(npoints), 0.0


def _check_rloess_windows(s, npoints, frac, degree, tiled, tile):
    """the checks of `rloess` that need the lengths of the selection `s` and no device -> the tile as the kernel takes it"""
    if frac:
        lo, hi = frac_points(s.min_len, frac), frac_points(s.max_len, frac)
        if lo < degree + 2:
            raise ValueError(f'npoints = {frac!r} gives a record of {s.min_len} samples a window of {lo}: degree {degree} needs {degree + 2} points')
        if hi > MAX_POINTS:
            raise ValueError(f'npoints = {frac!r} gives a record of {s.max_len} samples a window of {hi}: at most {MAX_POINTS} are supported')
    t = _check_tile(tiled, tile)
    if tiled:
        widest = min(frac_points(s.max_len, frac) if frac else npoints, s.max_len)
        if (t or LOESS_TILE) + 2 * widest > LOESS_LDS:
            raise ValueError(f'tile = {tile}: the tile and two windows of {widest} samples must fit {LOESS_LDS} samples of LDS (at most {LOESS_LDS - 2 * widest})')
        if -(-s.max_len // (t or LOESS_TILE)) > _MAX_TILES:
            raise ValueError(f'tile = {tile}: a record of {s.max_len} samples would need more than {_MAX_TILES} tiles')
    return t


def rloess(records, npoints=500, degree=2, robust_iters=10, subtract=False, offsets=None, idxs=None, out=None, chunk_records=None,
           return_iters=False, tiled=False, tile=None):
    """The reference's `rloess` (:61-73; `loess_1d(x, sig, degree=2, npoints=n)[1]`) for every lead of the selected records: the robust local
    regression baseline (include/ecgvit_hip.h states the algorithm and the two results defined here; parity with the `loess` package is
    unpinned).  f64 arithmetic.  npoints: an int, `degree + 2` to 1024 (a shorter record takes all its samples), or a float in (0, 1), the
    reference's fraction form: force_odd(int(n * npoints) - 1) per record of n samples.  robust_iters: 0 (the plain LOESS) to 10.
    subtract: write records - baseline (the difference in f64, rounded once) instead of the baseline.
    return_iters: -> (output, iters), iters an int8 (selected records, 12, longest selected record) table of the robust iterations run at each
    sample, rows in `idxs` order, 0 past a record's end (a device tensor for a device store, a numpy array for a host store).
    tiled: run `ecgvit_rloess_tiled` (records up to `MAX_LEN_TILED` samples; the bits and the iteration counts of the resident kernel for every
    record it takes and every tile).  tile: the output samples a workgroup owns (None: 2048); the tile and two windows must fit 4096 samples of
    LDS.  In place the tiled kernel runs through a scratch (the module's docstring says what it costs).  The iteration table is one byte per
    sample and lead of the selection (5.6 MB per record of 462 600 samples); a host store moves it to the host chunk by chunk."""
    npoints, frac = _check_rloess_args(npoints, degree, robust_iters)
    records, s = _resolve(records, offsets, idxs, degree + 2, tiled, unique=(True, True))
    tile = _check_rloess_windows(s, npoints, frac, degree, tiled, tile)
    on_device = isinstance(records, torch.Tensor)
    tail = (npoints, frac, int(degree), int(robust_iters), int(bool(subtract)))
    tables = []

    def stage(x, o, tab, first):
        it = torch.zeros((tab.R, C, tab.max_len), dtype=torch.int8, device=x.device) if return_iters else None
        if tiled:
            def launch(xs, os_, off, stride, lo, cnt):
                run.ecgvit_rloess_tiled(ptr(xs), ptr(os_), ptr(off), stride, ptr(tab.raw_len[lo:]), cnt, C, tab.min_len, tab.max_len, *tail,
                                        ptr(it[lo:]) if it is not None else None, tile, stream())
            _tiled_groups(x, o, tab, launch)
        else:
            run.ecgvit_rloess(ptr(x), ptr(o), ptr(tab.src_off), tab.stride, ptr(tab.raw_len), tab.R, C, tab.min_len, tab.max_len, *tail,
                              ptr(it), stream())
        if it is not None:
            it = it if tab.max_len == s.max_len else torch.nn.functional.pad(it, (0, s.max_len - tab.max_len))
            tables.append(it if on_device or not tiled else it.cpu())
    res = _sweep(records, s, out, chunk_records, stage)
    if not return_iters:
        return res
    iters = tables[0] if len(tables) == 1 else torch.cat(tables)
    return res, (iters if isinstance(res, torch.Tensor) else iters.cpu().numpy())


class EcgDenoiser:
    """`DataPreprocessor.zheng` as one call over a record store: low-pass, minus `baseline`, non-local means.

    `EcgDenoiser(fqs=500)(records, baseline='rloess')` is the reference's Python `zheng(sig, fqs)`: its low-pass is always designed for 500 Hz
    (`zheng` does not pass `fqs` on) and its LOESS window is `fqs` samples, so for another rate pass `loess_points=fqs` beside `fqs=500`;
    `EcgDenoiser(fqs=f)` with the record's own rate designs the low-pass as the MATLAB twin does (whose `smooth(..., 'rloess')` is another
    algorithm and is not built).  baseline: 'rloess' subtracts the robust LOESS fit of the low-passed lead over `loess_points` samples
    (None: `int(fqs)`, what `zheng` passes, checked against the 4 .. 1024 the kernel takes only when this baseline is asked for; `rloess` says
    what is defined here rather than pinned by the reference); a tensor in the store's own
    layout is subtracted at that place instead; None (the default) subtracts nothing."""

    def __init__(self, fqs=500, scale=1.5, search_width=None, patch_width=10, loess_points=None):
        _check_nlm(scale, search_width, patch_width)
        self.fqs, self.scale, self.search_width, self.patch_width = fqs, scale, search_width, patch_width
        if loess_points is not None:
            self._check_loess_points(loess_points)
        self.loess_points = int(fqs) if loess_points is None else loess_points     # the default is checked when baseline='rloess' asks for it
        self.b, self.a, self.zi = design_lowpass(fqs)

    @staticmethod
    def _check_loess_points(points):
        if isinstance(points, bool) or not isinstance(points, (int, np.integer)) or not 4 <= points <= MAX_POINTS:
            raise ValueError(f'loess_points = {points!r}: an int, 4 to {MAX_POINTS}')

    def __repr__(self):
        return f'<{self.__class__.__qualname__} fqs={self.fqs} scale={self.scale} search_width={self.search_width} patch_width={self.patch_width} loess_points={self.loess_points}>'

    def __call__(self, records, baseline=None, offsets=None, idxs=None, out=None, chunk_records=None, tiled=False, tile=None):
        """records: a float32 device store (-> device tensor), or a host array / memmap, streamed `chunk_records` records at a time through each
        stage (-> float32 numpy array; `baseline` is then a host array of the same shape).
        tiled, tile: every stage with `tiled=True` (records up to `MAX_LEN_TILED` samples); `tile` goes to the non-local means and the robust
        LOESS alike, so it is a multiple of 15 that fits the LOESS (the stages after the low-pass work in place: through a scratch)."""
        _check_tile(tiled, tile, NLM_RUN)
        loess = isinstance(baseline, str)
        if loess and baseline != 'rloess':
            raise ValueError(f"baseline = {baseline!r}: 'rloess' (the robust LOESS fit), a tensor in the store's layout, or None")
        # the one resolution, which every stage takes as its `idxs`; the low-pass needs the longest records of the three (13 samples at least)
        records, s = _resolve(records, offsets, idxs, 3 * max(len(self.a), len(self.b)) + 1, tiled, unique=(True, loess))
        device = isinstance(records, torch.Tensor)
        if loess:               # every check of the LOESS stage before the first stage touches the device
            self._check_loess_points(self.loess_points)
            _check_rloess_windows(s, self.loess_points, 0.0, 2, tiled, tile)
        if baseline is not None and not loess:
            ok = (isinstance(baseline, torch.Tensor) and baseline.dtype == torch.float32 and baseline.device == records.device) if device else \
                isinstance(baseline, (np.ndarray, torch.Tensor))
            if not ok or tuple(baseline.shape) != tuple(records.shape):
                raise ValueError("baseline must be in the store's layout: a float32 device tensor for a device store, a host array for a host store")
        out = lowpass_taps(records, self.b, self.a, self.zi, idxs=s, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)
        if loess:
            out = rloess(out, self.loess_points, subtract=True, idxs=s, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)
        elif baseline is not None:
            base = baseline if device else np.asarray(baseline, np.float32)
            if idxs is None:
                out -= base
            elif s.rect:
                ids = torch.from_numpy(s.sel).to(out.device) if device else s.sel
                out[ids] = out[ids] - base[ids]
            else:
                for src, l in zip(s.src_off.tolist(), s.raw_len.tolist()):
                    out[:, src:src + l] -= base[:, src:src + l]
        return nlm(out, self.scale, self.search_width, self.patch_width, idxs=s, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)
