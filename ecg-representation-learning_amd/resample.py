"""
The reference's export stage on the device: every corpus resampled to one rate (`RecDataExport.export_record_data`,
`preprocess/data_export.py:202-215`: `wfdb.processing.resample_sig(sig, fqs, 250)` per lead), the stage in front of `EcgDenoiser`,
`fit_dynamic_normalize` and `EcgTokenizer`, over the same record stores (`records.py`): (n, 12, L) float32 records, a ragged (12, S_total) store
with `offsets`, a subset `idxs` of either, a host array / memmap streamed `chunk_records` records at a time.  There is no CPU fallback.

`resample_sig` reduces to `scipy.signal.resample(x, num=int(n * fs_target / fs))`: Fourier resampling.  WHAT IS PINNED: the scipy call -- the
tests hold the kernels (`csrc/resample.hip`; include/ecgvit_hip.h states the algorithm in full) to a numpy f64 restatement of scipy's rule that
equals `scipy.signal.resample` on f64 input, and to a stored scipy output of the f32 input, which is what the reference's call computes.  WHAT
IS NOT: the `wfdb` wrapper is not available, so its length rule is restated (`resampled_length`), not executed.

It is the one stage whose output has another shape than its input, so it returns a NEW store and has no in-place form and no `out=`: a rectangle
gives (R, 12, L'), a ragged store gives ((12, S'), new_offsets) holding the selected records in `idxs` order (a repeat is a second copy), a host
array gives a host array.  A record's output has the same bits in every form, alone or in a batch.

Ragged records are grouped by length on the host: one plan, one pair of twiddle tables (16 bytes per sample of the length, made by numpy and
uploaded; 512 MiB at the cap of 1 << 25 samples) and one launch sequence per distinct length, and that again per record group of
`workspace_bytes`.  A launch sequence is 3 + passes(n_in) + passes(n_out) launches (5000 -> 2500: 9), so a store of D distinct lengths costs D
such sequences and D table uploads however few records share a length: a corpus of thousands of distinct lengths is launch-bound, and
cropping to a few lengths first is the caller's remedy.
Not built: Bluestein's algorithm (a prime length runs the dense DFT, O(n^2); a prime factor above 65 536 is refused), an LDS-resident fusion
of consecutive passes, NaN samples (wfdb interpolates them first: do that before), windowed resampling, the HDF5 writer.
"""
import ctypes

import numpy as np
import torch

from .records import RecordSelection, check_device_store, host_chunks, select_records

MAX_LEN = 1 << 25            # samples per record, before and after: the denoiser's Holter cap
MAX_GENERIC = 65536          # the widest prime factor a length may have (one generic-radix pass; above it the pass would run for minutes)
BUILT_RADICES = (25, 16, 8, 5, 4, 3, 2)
C = 12                       # leads per record: what `select_records` admits (the kernels pair them: lead 2p with lead 2p + 1)
_WS_BYTES = 2 ** 30          # the default of `workspace_bytes`: the two ping-pong buffers of a record group
_MAX_GROUP = 65535 // (C // 2)   # records per launch: the grid's second dimension holds record x lead pair


def resampled_length(n, fqs, fqs_target):
    """the length `wfdb.processing.resample_sig` gives a lead of n samples: int(n * fqs_target / fqs), in Python arithmetic (the reference's
    expression, restated).  n < 1 or a result below 1 raises ValueError."""
    if n < 1:
        raise ValueError(f'a record of {n} samples')
    if not (fqs > 0 and fqs_target > 0):
        raise ValueError(f'fqs = {fqs!r}, fqs_target = {fqs_target!r}: positive rates')
    num = int(n * fqs_target / fqs)
    if num < 1:
        raise ValueError(f'a record of {n} samples at {fqs} Hz resamples to {num} samples at {fqs_target} Hz')
    return num


def plan(n):
    """the radices of the passes of a transform of length n (`ecgvit_resample_plan`: host only): the built radices 25, 16, 8, 5, 4, 3, 2
    largest first, then every other prime factor, one generic pass each; [] for n == 1"""
    from .hip import lib
    rad = (ctypes.c_int * 32)()
    cnt = lib().ecgvit_resample_plan(int(n), rad, 32)
    if cnt < 0:
        raise ValueError(f'a record of {n} samples: 1 to {MAX_LEN} are supported')
    return list(rad[:cnt])


def _check_length(n):
    wide = [r for r in plan(n) if r not in BUILT_RADICES and r > MAX_GENERIC]
    if wide:
        raise ValueError(f'a record of {n} samples has the prime factor {wide[0]}: above {MAX_GENERIC} its dense pass is not run (Bluestein is not built)')


def twiddles(n, sign):
    """exp(sign * 2 pi i k / n), k < n, as an (n, 2) float64 array: the table `ecgvit_resample` takes for a length (sign -1: forward, +1: inverse)"""
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.ascontiguousarray(np.stack([np.cos(ang), sign * np.sin(ang)], axis=-1))


def _offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _copy_records(x, out, src, s_stride, dst, d_stride, n):
    """records of n samples from x to out, bit for bit (torch indexing: plumbing, no arithmetic)"""
    fx, fo = x.view(-1), out.view(-1)
    ar = torch.arange(n, device=x.device)
    si = (torch.from_numpy(src).to(x.device)[:, None] + ar).reshape(-1)
    di = (torch.from_numpy(dst).to(x.device)[:, None] + ar).reshape(-1)
    for c in range(C):
        fo[di + c * d_stride] = fx[si + c * s_stride]


def _run(x, src_off, lens, s_stride, out, dst_off, out_lens, d_stride, ws_bytes, tables):
    """resample the records (src_off, lens) of the device store x into (dst_off, out_lens) of the device store out: grouped by length, then by
    workspace.  tables: {(n, sign): device table}, kept over the chunks of one call."""
    from .hip import lib, check, ptr, stream
    pairs = np.stack([lens, out_lens], axis=1)
    for n_in, n_out in np.unique(pairs, axis=0).tolist():
        g = np.nonzero((lens == n_in) & (out_lens == n_out))[0]
        src, dst = np.ascontiguousarray(src_off[g]), np.ascontiguousarray(dst_off[g])
        if n_in == n_out:
            _copy_records(x, out, src, s_stride, dst, d_stride, n_in)
            continue
        need = lib().ecgvit_resample_workspace(1, C, n_in, n_out)
        step = min(ws_bytes // need, _MAX_GROUP, len(g))
        if step < 1:
            raise ValueError(f'workspace_bytes = {ws_bytes}: one record of {n_in} -> {n_out} samples needs {need}')
        for key in ((n_in, -1), (n_out, 1)):
            if key not in tables:
                tables[key] = torch.from_numpy(twiddles(*key)).to(x.device)
        ws = torch.empty(step * need // 8, dtype=torch.float64, device=x.device)
        src_d, dst_d = torch.from_numpy(src).to(x.device), torch.from_numpy(dst).to(x.device)
        for lo in range(0, len(g), step):
            cnt = min(step, len(g) - lo)
            check(lib().ecgvit_resample(ptr(x), ptr(out), ptr(src_d[lo:]), s_stride, ptr(dst_d[lo:]), d_stride, cnt, C, n_in, n_out,
                                        ptr(tables[(n_in, -1)]), ptr(tables[(n_out, 1)]), ptr(ws), stream()), 'ecgvit_resample')


def resample(records, fqs, fqs_target=250, num=None, offsets=None, idxs=None, chunk_records=None, workspace_bytes=None):
    """`scipy.signal.resample(lead, resampled_length(n, fqs, fqs_target))` for every lead of the selected records (f64 arithmetic, f32 loads and
    stores), into a new store: (R, 12, L') for a rectangle, ((12, S'), new_offsets) for a ragged store (new_offsets an int64 numpy table,
    the cumulative `resampled_length` in `idxs` order), a float32 numpy array (or pair) for a host array / memmap.
    fqs == fqs_target returns a bit-equal copy of the selected records, as wfdb does (no FFT round trip).
    num: the output length of a rectangle, instead of the rates' (a ragged store refuses it); num == L copies too.
    chunk_records: records per upload of a host store (None: about 256 MB of f32).
    workspace_bytes: the limit of the two complex f64 ping-pong buffers of a record group (None: 1 GiB; 32 bytes per sample and lead of the
    longer side, so a record of 462 600 samples needs 89 MB); more records run in several groups, and a single record that needs more raises
    with the number it needs.
    Launches: one sequence of 3 + passes(n_in) + passes(n_out) per distinct length and record group (the module's docstring says what a store
    of many distinct lengths costs).  NaN samples are not supported."""
    on_device = isinstance(records, torch.Tensor) and records.is_cuda
    if isinstance(records, torch.Tensor) and not on_device:
        raise ValueError('records must be a float32 device tensor, or a host array / memmap (a CPU tensor is neither: pass .numpy() or .cuda())')
    if on_device:
        check_device_store(records)
    elif not hasattr(records, 'shape') or not hasattr(records, 'dtype') or not np.issubdtype(records.dtype, np.floating):
        raise ValueError('records must be a float32 device tensor or a host array / memmap of a float type')
    s = idxs if isinstance(idxs, RecordSelection) else select_records(records, offsets, idxs)
    if s.C % 2:
        raise ValueError(f'records must hold an even number of leads, got {s.C}')
    if num is not None:
        if not s.rect:
            raise ValueError('num= gives one length: a ragged store takes its lengths from the rates')
        if isinstance(num, bool) or not isinstance(num, (int, np.integer)) or num < 1:
            raise ValueError(f'num = {num!r}: an int, at least 1')
    if not (fqs > 0 and fqs_target > 0):
        raise ValueError(f'fqs = {fqs!r}, fqs_target = {fqs_target!r}: positive rates')
    if s.max_len > MAX_LEN:
        raise ValueError(f'a record of {s.max_len} samples: at most {MAX_LEN} are supported')
    lens = s.raw_len
    if num is not None:
        out_lens = np.full(s.R, int(num), np.int64)
    elif fqs == fqs_target:
        out_lens = lens.copy()
    else:
        by_len = {int(n): resampled_length(int(n), fqs, fqs_target) for n in np.unique(lens)}
        out_lens = np.array([by_len[int(n)] for n in lens], np.int64)
    if int(out_lens.max()) > MAX_LEN:
        raise ValueError(f'a record resamples to {int(out_lens.max())} samples: at most {MAX_LEN} are supported')
    for n in np.unique(np.concatenate([lens[lens != out_lens], out_lens[lens != out_lens]])):
        _check_length(int(n))
    ws_bytes = _WS_BYTES if workspace_bytes is None else int(workspace_bytes)
    if ws_bytes < 1:
        raise ValueError(f'workspace_bytes = {workspace_bytes!r}: a positive number of bytes')
    new_off = _offsets_of(out_lens)

    def layout(first, cnt):
        """the destination tables of the records first .. first + cnt of the selection in a compact store of their own -> (shape, dst_off, stride)"""
        if s.rect:
            L = int(out_lens[0])
            return (cnt, C, L), np.arange(cnt, dtype=np.int64) * (C * L), L
        off = new_off[first:first + cnt] - new_off[first]
        S = int(new_off[first + cnt] - new_off[first])
        return (C, S), off, S

    tables = {}
    if on_device:
        shape, dst_off, d_stride = layout(0, s.R)
        with torch.cuda.device(records.device):
            out = torch.empty(shape, dtype=torch.float32, device=records.device)
            _run(records, s.src_off, lens, s.stride, out, dst_off, out_lens, d_stride, ws_bytes, tables)
        return out if s.rect else (out, new_off)
    chunks = host_chunks(records, s, chunk_records)
    if not torch.cuda.is_available():
        raise RuntimeError('resample runs on the device (no CPU fallback exists)')
    out = np.empty(layout(0, s.R)[0], np.float32)
    device = torch.device('cuda')
    first = 0
    with torch.cuda.device(device):
        for buf, off, clens, stride, _ in chunks:
            cnt = len(clens)
            shape, dst_off, d_stride = layout(first, cnt)
            x = torch.from_numpy(buf).to(device)
            o = torch.empty(shape, dtype=torch.float32, device=device)
            _run(x, np.asarray(off, np.int64), np.asarray(clens, np.int64), int(stride), o, dst_off, out_lens[first:first + cnt], d_stride, ws_bytes, tables)
            if s.rect:
                out[first:first + cnt] = o.cpu().numpy()
            else:
                out[:, new_off[first]:new_off[first + cnt]] = o.cpu().numpy()
            first += cnt
    return out if s.rect else (out, new_off)
