"""
The reference's Zheng et al. denoiser (`ecg_transformer/preprocess/data_preprocessor.py:22-148`, MATLAB twin `preprocess_matlab/DataPreprocessor.m`
and `nlm.m`) on the device: zero-phase Butterworth low-pass, the robust LOESS baseline it subtracts, the noise estimate and non-local means,
the stage that writes the `*-denoised.hdf5` files every reference run trains on.  The sweeps are HIP kernels (`csrc/denoise.hip`) over the record stores `fit_dynamic_normalize` and
`EcgTokenizer` take: (n, 12, L) float32 records, a ragged (12, S_total) store with `offsets`, a subset `idxs` of either.  A device store is
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

from .transform import _record_tables

MAX_LEN = 32768            # samples per record: the resident non-local means and LOESS keep a lead in LDS
MAX_LEN_TILED = 1 << 25    # samples per record with tiled=True (24 hours at 360 Hz)
NLM_RUN = 15               # output samples per run of the non-local means: `tile` is a multiple of it there
NLM_TILE = 512 * NLM_RUN   # the default tile of the non-local means: one run per lane of a 512-lane workgroup
LOESS_LDS = 4096           # samples the tiled LOESS keeps in LDS: a tile and two windows
LOESS_TILE = LOESS_LDS - 2 * 1024      # its default tile
_MAX_TILES = 65535         # tiles per lead (the grid's third dimension)
MAX_TAPS = 9
MAX_POINTS = 1024          # samples per LOESS window: covers every sampling rate of the reference's config (250, 257, 500, 1000)
MAX_ROBUST_ITERS = 10
C = 12                     # leads per record: what `_record_tables` admits
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
class _Tables:
    """the device tables of the selected records of one device store"""

    def __init__(self, x, src_off, raw_len, stride):
        self.x, self.R, self.stride = x, len(raw_len), int(stride)
        self.src_off_h, self.raw_len_h = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(raw_len, np.int64)
        self.src_off = torch.from_numpy(self.src_off_h.copy()).to(x.device)
        self.raw_len = torch.from_numpy(self.raw_len_h.astype(np.int32)).to(x.device)
        self.min_len, self.max_len = int(self.raw_len_h.min()), int(self.raw_len_h.max())

    def launches(self, tiled=False):
        """(first record, records) per launch, so that the f64 workspace of a launch stays within _WS_BYTES"""
        from .hip import lib
        size = lib().ecgvit_denoise_workspace_long if tiled else lib().ecgvit_denoise_workspace
        step = max(1, _WS_BYTES // size(1, C, self.max_len))
        return [(lo, min(step, self.R - lo)) for lo in range(0, self.R, step)]

    def groups(self):
        """(first record, records) per launch group of a tiled stage that runs in place: each of the group's two f32 scratch stores stays within
        _WS_BYTES (at 462 600 samples: 12 records)"""
        step = max(1, _WS_BYTES // (4 * C * self.max_len))
        return [(lo, min(step, self.R - lo)) for lo in range(0, self.R, step)]

    def compact(self, lo, cnt):
        """the records lo .. lo + cnt as a compact (12, S) store -> (its offsets as a device table, S, the store column of every compact column)"""
        lens, src = self.raw_len_h[lo:lo + cnt], self.src_off_h[lo:lo + cnt]
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        S = int(lens.sum())
        cols = np.repeat(src - off, lens) + np.arange(S, dtype=np.int64)
        return torch.from_numpy(off).to(self.x.device), S, torch.from_numpy(cols).to(self.x.device)


def _tiled_groups(x, o, tab, launch):
    """Run `launch(x, out, src_off table of the launch's records, lead stride, first record, records)` of a tiled kernel over the records of `tab`.
    Out of place: one launch on the store itself.  In place (the kernels refuse out == x): group by group through two compact scratch stores."""
    if o.data_ptr() != x.data_ptr():
        launch(x, o, tab.src_off, tab.stride, 0, tab.R)
        return
    flat_x, flat_o = x.view(-1), o.view(-1)
    for lo, cnt in tab.groups():
        off, S, cols = tab.compact(lo, cnt)
        a = torch.stack([flat_x[cols + c * tab.stride] for c in range(C)])
        b = a.clone()           # (a lead the kernel leaves alone keeps its samples)
        launch(a, b, off, S, lo, cnt)
        for c in range(C):
            flat_o[cols + c * tab.stride] = b[c]


def _check_device_store(records, what='records'):
    if records.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {records.dtype}')
    if not records.is_cuda:
        raise ValueError(f'{what} must be a device tensor or a host array (a host TENSOR is taken as a host array only as `records`)')
    if not records.is_contiguous():
        raise ValueError(f'{what} must be contiguous')


def _check_lengths(raw_len, min_len=1, tiled=False):
    if tiled and int(raw_len.max()) > MAX_LEN_TILED:
        raise ValueError(f'a record of {int(raw_len.max())} samples: at most {MAX_LEN_TILED} are supported with tiled=True')
    if not tiled and int(raw_len.max()) > MAX_LEN:
        raise ValueError(f'a record of {int(raw_len.max())} samples: at most {MAX_LEN} are supported (tiled=True takes up to {MAX_LEN_TILED})')
    if int(raw_len.min()) < min_len:
        raise ValueError(f'a record of {int(raw_len.min())} samples: this stage needs at least {min_len}')


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
    _check_device_store(out, 'out')
    if out.shape != records.shape or out.device != records.device:
        raise ValueError(f'out must have the shape and device of records, got {tuple(out.shape)} on {out.device}')
    if out.data_ptr() == records.data_ptr():
        return out
    lo, hi = records.data_ptr(), records.data_ptr() + records.numel() * 4
    if out.data_ptr() < hi and lo < out.data_ptr() + out.numel() * 4:
        raise ValueError('out overlaps records without being records: pass out=records to run in place')
    return out


def _host_chunks(records, rect, src_off, raw_len, sel, chunk_records, device):
    """-> per chunk (device buffer, _Tables, scatter): the selected records, `chunk_records` at a time, as a compact device store of the same form;
    scatter(host_out, buffer) writes the chunk's records back where they came from"""
    if chunk_records is None:   # about 256 MB of f32 per chunk
        chunk_records = max(1, int(64 * 2 ** 20 // (C * max(1, int(raw_len.max())))))
    step = int(chunk_records)
    for lo in range(0, len(sel), step):
        ids, lens, srcs = sel[lo:lo + step], raw_len[lo:lo + step], src_off[lo:lo + step]
        if rect:
            L = int(lens[0])
            buf = np.ascontiguousarray(records[ids], dtype=np.float32)
            off, stride = np.arange(len(ids), dtype=np.int64) * (C * L), L

            def scatter(host_out, dev, ids=ids):
                host_out[ids] = dev.cpu().numpy()
        else:
            S = int(lens.sum())
            buf = np.empty((C, S), np.float32)
            off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
            for o, s, l in zip(off.tolist(), srcs.tolist(), lens.tolist()):
                buf[:, o:o + l] = records[:, s:s + l]
            stride = S

            def scatter(host_out, dev, off=off, srcs=srcs, lens=lens):
                h = dev.cpu().numpy()
                for o, s, l in zip(off.tolist(), srcs.tolist(), lens.tolist()):
                    host_out[:, s:s + l] = h[:, o:o + l]
        x = torch.from_numpy(buf).to(device)
        yield x, _Tables(x, off, lens, stride), scatter


def _sweep(records, offsets, idxs, out, chunk_records, min_len, stage, tables=None, tiled=False):
    """Run `stage(x, out, tables, first selected record)` over the selected records.  Device store: one call, returns the output tensor.  Host
    store: chunk by chunk in place on a staging buffer, returns a float32 numpy array (a copy of the input with the selected records replaced;
    `out`, a float32 array of the same shape, is filled instead when given).  tables: what `_record_tables` gave a caller that had to check the
    selection before (the lengths are then the caller's to check)."""
    if isinstance(records, torch.Tensor) and records.is_cuda:
        _check_device_store(records)
        rect, n, _, src_off, raw_len, stride, sel = tables or _record_tables(records, offsets, idxs)
        if tables is None:
            _check_lengths(raw_len, min_len, tiled)
        if len(np.unique(sel)) != len(sel):
            raise ValueError('idxs repeats a record: two workgroups would write the same samples')
        out = _resolve_out(records, out)
        with torch.cuda.device(records.device):
            stage(records, out, _Tables(records, src_off, raw_len, stride), 0)
        return out
    host = records.numpy() if isinstance(records, torch.Tensor) else records
    if not hasattr(host, 'shape') or not hasattr(host, 'dtype') or not np.issubdtype(host.dtype, np.floating):
        raise ValueError('records must be a float32 device tensor or a host array / memmap / tensor of a float type')
    rect, n, _, src_off, raw_len, stride, sel = tables or _record_tables(host, offsets, idxs)
    if tables is None:
        _check_lengths(raw_len, min_len, tiled)
    if out is not None and out is not False:
        if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != host.shape:
            raise ValueError('for a host store, out must be a float32 numpy array of the same shape')
    if chunk_records is not None and int(chunk_records) < 1:
        raise ValueError('chunk_records must be at least 1')
    if not torch.cuda.is_available():
        raise RuntimeError('the denoiser runs on the device (no CPU fallback exists)')
    if out is None:
        out = np.array(host, dtype=np.float32)
    device = torch.device('cuda')
    first = 0
    with torch.cuda.device(device):
        for x, tab, scatter in _host_chunks(host, rect, src_off, raw_len, sel, chunk_records, device):
            stage(x, x, tab, first)
            if out is not False:
                scatter(out, x)
            first += tab.R
    return out


# ---- the three stages -----------------------------------------------------------------------------------------------------------------
def _workspace(tab, device, tiled=False):
    from .hip import lib
    R = max(cnt for _, cnt in tab.launches(tiled))
    size = lib().ecgvit_denoise_workspace_long if tiled else lib().ecgvit_denoise_workspace
    return torch.empty(size(R, C, tab.max_len) // 8, dtype=torch.float64, device=device)


def lowpass_taps(records, b, a, zi=None, offsets=None, idxs=None, out=None, chunk_records=None, tiled=False, tile=None):
    """`scipy.signal.filtfilt(b, a, lead)` with its defaults for every lead of the selected records (f64 arithmetic; odd extension by
    3 * max(len(a), len(b)) samples, which every record must exceed).  zi: `lfilter_zi(b, a)` when None.
    tiled: run `ecgvit_filtfilt_long` (the same kernel, records up to `MAX_LEN_TILED` samples, the same bits); `tile` is checked and ignored --
    the recurrence is walked by one lane per lead whatever the length, and runs in place without a scratch."""
    from .hip import lib, check, ptr, stream
    b, a, zi, nt = _taps(b, a, zi)
    _check_tile(tiled, tile)

    def stage(x, o, tab, first):
        ws = _workspace(tab, x.device, tiled)
        fn, name = (lib().ecgvit_filtfilt_long, 'ecgvit_filtfilt_long') if tiled else (lib().ecgvit_filtfilt, 'ecgvit_filtfilt')
        for lo, cnt in tab.launches(tiled):
            check(fn(ptr(x), ptr(o), ptr(tab.src_off[lo:]), tab.stride, ptr(tab.raw_len[lo:]), cnt, C, tab.min_len, tab.max_len,
                     _dp(b), _dp(a), _dp(zi), nt, ptr(ws), stream()), name)
    return _sweep(records, offsets, idxs, out, chunk_records, 3 * nt + 1, stage, tiled=tiled)


def lowpass(records, fqs=500, passband=50, stopband=60, passband_ripple=1, stopband_attenuation=2.5, offsets=None, idxs=None, out=None,
            chunk_records=None, tiled=False, tile=None):
    """The reference's `butterworth_low_pass` (:48-58): `design_lowpass` then the zero-phase filter.  The reference's `zheng` never passes its
    `fqs` on, so it always filters with the 500 Hz design; the MATLAB twin passes it.  Here `fqs` is explicit.  tiled, tile: `lowpass_taps`."""
    b, a, zi = design_lowpass(fqs, passband, stopband, passband_ripple, stopband_attenuation)
    return lowpass_taps(records, b, a, zi, offsets=offsets, idxs=idxs, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)


def estimate_noise_std(records, offsets=None, idxs=None, chunk_records=None, tiled=False, tile=None):
    """The reference's `est_noise_std` (:76-80) for every lead of the selected records -> (R, 12) float64 device tensor, rows in `idxs` order.
    tiled: run `ecgvit_nlm_sigma_long` (the same kernel, records up to `MAX_LEN_TILED` samples, the same bits); `tile` is checked and ignored."""
    tables = []
    _check_tile(tiled, tile)

    def stage(x, o, tab, first):
        sig = _sigma_of(x, tab, tiled)
        tables.append(sig)
    if isinstance(records, torch.Tensor) and records.is_cuda:
        _check_device_store(records)
        rect, n, _, src_off, raw_len, stride, sel = _record_tables(records, offsets, idxs)
        _check_lengths(raw_len, 1, tiled)
        with torch.cuda.device(records.device):
            stage(records, None, _Tables(records, src_off, raw_len, stride), 0)
    else:
        _sweep(records, offsets, idxs, False, chunk_records, 1, stage, tiled=tiled)
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
    from .hip import lib, check, ptr, stream
    _check_nlm(scale, search_width, patch_width)
    tile_runs = _check_tile(tiled, tile, NLM_RUN) // NLM_RUN
    if sigma is not None:
        if isinstance(sigma, np.ndarray):
            sigma = torch.from_numpy(np.ascontiguousarray(sigma, np.float64))
        if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float64 or sigma.dim() != 2 or sigma.shape[1] != 12:
            raise ValueError('sigma must be an (R, 12) float64 table, one row per selected record')

    def stage(x, o, tab, first):
        if sigma is None:
            sig = _sigma_of(x, tab, tiled)
        else:
            sig = sigma[first:first + tab.R].to(x.device).contiguous()
        if tiled:
            runs = max(1, -(-(tab.max_len - 2 * int(patch_width) - 1) // NLM_RUN))
            if -(-runs // min(tile_runs or NLM_TILE // NLM_RUN, runs)) > _MAX_TILES:
                raise ValueError(f'tile = {tile}: a record of {tab.max_len} samples would need more than {_MAX_TILES} tiles')

            def launch(xs, os_, off, stride, lo, cnt):
                check(lib().ecgvit_nlm_denoise_tiled(ptr(xs), ptr(os_), ptr(off), stride, ptr(tab.raw_len[lo:]), cnt, C,
                                                     tab.max_len, ptr(sig[lo:]), float(scale), int(patch_width),
                                                     0 if search_width is None else int(search_width), tile_runs, stream()), 'ecgvit_nlm_denoise_tiled')
            return _tiled_groups(x, o, tab, launch)
        check(lib().ecgvit_nlm_denoise(ptr(x), ptr(o), ptr(tab.src_off), tab.stride, ptr(tab.raw_len), tab.R, C, tab.max_len, ptr(sig), float(scale),
                                       int(patch_width), 0 if search_width is None else int(search_width), stream()), 'ecgvit_nlm_denoise')
    if sigma is not None:
        n_sel = _selected(records, offsets, idxs)
        if sigma.shape[0] != n_sel:
            raise ValueError(f'sigma holds {sigma.shape[0]} rows for {n_sel} selected records')
    return _sweep(records, offsets, idxs, out, chunk_records, 1, stage, tiled=tiled)


def frac_points(n, frac):
    """the window the reference's `rloess` gives a record of n samples for a float `n`: force_odd(int(sig.size * n) - 1)"""
    return 2 * math.floor((int(n * frac) - 1) / 2) + 1


def _check_rloess(records, npoints, degree, robust_iters, offsets, idxs, tiled=False, tile=None):
    """every check of `rloess` that needs no device -> (npoints as the kernel takes it, the fraction or 0.0, the `_record_tables` of the selection)"""
    if isinstance(degree, bool) or not isinstance(degree, (int, np.integer)) or degree not in (1, 2):
        raise ValueError(f'degree = {degree!r}: 1 or 2')
    if isinstance(robust_iters, bool) or not isinstance(robust_iters, (int, np.integer)) or not 0 <= robust_iters <= MAX_ROBUST_ITERS:
        raise ValueError(f'robust_iters = {robust_iters!r}: an int, 0 to {MAX_ROBUST_ITERS}')
    frac = 0.0
    if isinstance(npoints, (float, np.floating)):
        if not 0.0 < npoints < 1.0:
            raise ValueError(f'npoints = {npoints!r}: a fraction lies in (0, 1)')
        frac, npoints = float(npoints), 0
    elif isinstance(npoints, bool) or not isinstance(npoints, (int, np.integer)) or not degree + 2 <= npoints <= MAX_POINTS:
        raise ValueError(f'npoints = {npoints!r}: an int, {degree + 2} (degree + 2) to {MAX_POINTS}, or a fraction in (0, 1)')
    host = records.numpy() if isinstance(records, torch.Tensor) and not records.is_cuda else records
    if isinstance(host, torch.Tensor):
        _check_device_store(host)
    elif not hasattr(host, 'shape') or not hasattr(host, 'dtype') or not np.issubdtype(host.dtype, np.floating):
        raise ValueError('records must be a float32 device tensor or a host array / memmap / tensor of a float type')
    tabs = _record_tables(host, offsets, idxs)
    raw_len, sel = tabs[4], tabs[6]
    if len(np.unique(sel)) != len(sel):
        raise ValueError('idxs repeats a record: two workgroups would write the same samples')
    _check_lengths(raw_len, degree + 2, tiled)
    if frac:
        lo, hi = frac_points(int(raw_len.min()), frac), frac_points(int(raw_len.max()), frac)
        if lo < degree + 2:
            raise ValueError(f'npoints = {frac!r} gives a record of {int(raw_len.min())} samples a window of {lo}: degree {degree} needs {degree + 2} points')
        if hi > MAX_POINTS:
            raise ValueError(f'npoints = {frac!r} gives a record of {int(raw_len.max())} samples a window of {hi}: at most {MAX_POINTS} are supported')
    t = _check_tile(tiled, tile) or LOESS_TILE
    if tiled:
        longest = int(raw_len.max())
        widest = min(frac_points(longest, frac) if frac else int(npoints), longest)
        if t + 2 * widest > LOESS_LDS:
            raise ValueError(f'tile = {tile}: the tile and two windows of {widest} samples must fit {LOESS_LDS} samples of LDS (at most {LOESS_LDS - 2 * widest})')
        if -(-longest // t) > _MAX_TILES:
            raise ValueError(f'tile = {tile}: a record of {longest} samples would need more than {_MAX_TILES} tiles')
    return int(npoints), frac, tabs


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
    from .hip import lib, check, ptr, stream
    npoints, frac, tabs = _check_rloess(records, npoints, degree, robust_iters, offsets, idxs, tiled, tile)
    tile = 0 if tile is None else int(tile)
    on_device = isinstance(records, torch.Tensor) and records.is_cuda
    raw_len = tabs[4]
    width = int(raw_len.max())
    tables = []

    def stage(x, o, tab, first):
        it = torch.zeros((tab.R, C, tab.max_len), dtype=torch.int8, device=x.device) if return_iters else None
        if tiled:
            def launch(xs, os_, off, stride, lo, cnt):
                check(lib().ecgvit_rloess_tiled(ptr(xs), ptr(os_), ptr(off), stride, ptr(tab.raw_len[lo:]), cnt, C,
                                                tab.min_len, tab.max_len, int(npoints), frac, int(degree), int(robust_iters), int(bool(subtract)),
                                                ptr(it[lo:]) if it is not None else None, tile, stream()), 'ecgvit_rloess_tiled')
            _tiled_groups(x, o, tab, launch)
        else:
            check(lib().ecgvit_rloess(ptr(x), ptr(o), ptr(tab.src_off), tab.stride, ptr(tab.raw_len), tab.R, C, tab.min_len, tab.max_len, int(npoints),
                                      frac, int(degree), int(robust_iters), int(bool(subtract)), ptr(it), stream()), 'ecgvit_rloess')
        if it is not None:
            it = it if tab.max_len == width else torch.nn.functional.pad(it, (0, width - tab.max_len))
            tables.append(it if on_device or not tiled else it.cpu())
    res = _sweep(records, offsets, idxs, out, chunk_records, degree + 2, stage, tables=tabs)
    if not return_iters:
        return res
    iters = tables[0] if len(tables) == 1 else torch.cat(tables)
    return res, (iters if isinstance(res, torch.Tensor) else iters.cpu().numpy())


def _sigma_of(x, tab, tiled=False):
    """the noise estimate over exactly the records of `tab` (a device store)"""
    from .hip import lib, check, ptr, stream
    sig = torch.zeros((tab.R, C), dtype=torch.float64, device=x.device)
    ws = _workspace(tab, x.device, tiled)
    fn, name = (lib().ecgvit_nlm_sigma_long, 'ecgvit_nlm_sigma_long') if tiled else (lib().ecgvit_nlm_sigma, 'ecgvit_nlm_sigma')
    for lo, cnt in tab.launches(tiled):
        check(fn(ptr(x), ptr(tab.src_off[lo:]), tab.stride, ptr(tab.raw_len[lo:]), cnt, C, tab.max_len, ptr(sig[lo:]), ptr(ws), stream()), name)
    return sig


def _selected(records, offsets, idxs):
    host = records.numpy() if isinstance(records, torch.Tensor) and not records.is_cuda else records
    return len(_record_tables(host, offsets, idxs)[6])


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
        device = isinstance(records, torch.Tensor) and records.is_cuda
        rect, n, _, src_off, raw_len, stride, sel = _record_tables(records.numpy() if isinstance(records, torch.Tensor) and not device else records, offsets, idxs)
        loess = isinstance(baseline, str)
        if loess and baseline != 'rloess':
            raise ValueError(f"baseline = {baseline!r}: 'rloess' (the robust LOESS fit), a tensor in the store's layout, or None")
        if loess:               # every check of the LOESS stage before the first stage touches the device
            self._check_loess_points(self.loess_points)
            _check_rloess(records, self.loess_points, 2, MAX_ROBUST_ITERS, offsets, idxs, tiled, tile)
        if baseline is not None and not loess:
            ok = (isinstance(baseline, torch.Tensor) and baseline.dtype == torch.float32 and baseline.device == records.device) if device else \
                isinstance(baseline, (np.ndarray, torch.Tensor))
            if not ok or tuple(baseline.shape) != tuple(records.shape):
                raise ValueError("baseline must be in the store's layout: a float32 device tensor for a device store, a host array for a host store")
        out = lowpass_taps(records, self.b, self.a, self.zi, offsets=offsets, idxs=idxs, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)
        if loess:
            out = rloess(out, self.loess_points, subtract=True, offsets=offsets, idxs=idxs, out=out, chunk_records=chunk_records, tiled=tiled, tile=tile)
        elif baseline is not None:
            base = baseline if device else np.asarray(baseline, np.float32)
            if idxs is None:
                out -= base
            elif rect:
                ids = torch.from_numpy(sel).to(out.device) if device else sel
                out[ids] = out[ids] - base[ids]
            else:
                for s, l in zip(src_off.tolist(), raw_len.tolist()):
                    out[:, s:s + l] -= base[:, s:s + l]
        return nlm(out, self.scale, self.search_width, self.patch_width, offsets=offsets, idxs=idxs, out=out, chunk_records=chunk_records, tiled=tiled,
                   tile=tile)
