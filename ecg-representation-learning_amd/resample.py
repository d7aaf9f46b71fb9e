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

Lengths with a wide prime factor (`chirp=`, opt-in): a prime factor r outside the built radices runs one generic pass whose cost grows with r,
a prime length runs the dense DFT, O(n^2), and a prime factor above 65 536 is refused.  With `chirp=r0` (or `chirp=True`: r0 = CHIRP_DEFAULT)
a length whose plan holds a generic radix >= r0 is transformed as a whole by Bluestein's algorithm instead (the chirp route of
include/ecgvit_hip.h: the exact DFT as a circular convolution of the smooth length M = `resample_chirp_length(n)` >= 2 n - 1, on the same
passes, O(n log n)), and a wide prime factor is refused only above 1 << 24 samples.  Every other length keeps its plain passes and its bits, and
the two sides of a resample choose independently.  What a distinct length on the chirp route costs beside the above: one extra M-transform on
the device (its filter spectrum, once per call and (length, direction)) and two more uploads (the chirp table of n entries and the twiddle table
of M, which lengths that share an M share); its launch sequence runs 2 passes(M) + 1 launches for that side and its workspace counts M, about
2 to 4 times n, for that side.  CHIRP_DEFAULT = 61 is read off profiles/r24_resample_chirp.txt (tools/resample_rate.py --chirp): 512 x 12 x 4 999 -> 2 499 takes 190 ms of
launches on the dense route and 2.6 ms with the input side on the chirp route; one record of 131 101 -> 65 550 samples, refused before, 0.35 ms.
Not built: the chirp route above 1 << 24 samples, a Rader or Bluestein pass for one factor inside a mixed plan (a length on the chirp route is
transformed whole), one launch sequence for many distinct lengths, an LDS-resident fusion of consecutive passes, NaN samples (wfdb
interpolates them first: do that before), windowed resampling, the HDF5 writer.
"""
import ctypes

import numpy as np
import torch

from . import hip
from .hip import lib, run, ptr, stream
from .records import RecordSelection, check_device_store, host_chunks, select_records

MAX_LEN = hip.RESAMPLE_MAX_LEN            # samples per record, before and after: the denoiser's Holter cap
MAX_GENERIC = hip.RESAMPLE_MAX_GENERIC    # the widest prime factor a length may have (one generic-radix pass; above it the pass would run for minutes)
MAX_CHIRP = hip.RESAMPLE_MAX_CHIRP        # samples of a length on the chirp route: its M stays within MAX_LEN
# r0 of `chirp=True`, read off profiles/r24_resample_chirp.txt (tools/resample_rate.py --chirp): the smallest tabled prime from which the chirp
# route beats the generic pass at both measured shapes (512 records near 5 000 samples: 3.67 against 2.16 ms; one record near 460 000: 1.75
# against 0.63 ms); at 31 it still loses at the short shape (2.42 against 3.48 ms) and about draws at the long one (0.99 against 0.93 ms)
CHIRP_DEFAULT = 61
BUILT_RADICES = (25, 16, 8, 5, 4, 3, 2)
C = 12                       # leads per record: what `select_records` admits (the kernels pair them: lead 2p with lead 2p + 1)
_WS_BYTES = 2 ** 30          # the default of `workspace_bytes`: the two ping-pong buffers of a record group
_MAX_GROUP = hip.RESAMPLE_MAX_GRID_Y // (C // 2)   # records per launch: the grid's second dimension holds record x lead pair


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
    rad = (ctypes.c_int * 32)()
    cnt = lib().ecgvit_resample_plan(int(n), rad, 32)
    if cnt < 0:
        raise ValueError(f'a record of {n} samples: 1 to {MAX_LEN} are supported')
    return list(rad[:cnt])


def chirp_length(n):
    """M of the chirp route for a length n (`ecgvit_resample_chirp_length`: host only): the smallest 2^a 3^b 5^c >= 2 n - 1; -1 for n < 1 or
    n > 1 << 24"""
    return int(lib().ecgvit_resample_chirp_length(int(n)))


def _chirp_r0(chirp):
    """`chirp=` -> r0, or None for today's routes"""
    if chirp is None or chirp is False:
        return None
    if chirp is True:
        return CHIRP_DEFAULT
    if not isinstance(chirp, (int, np.integer)) or chirp < 7:
        raise ValueError(f'chirp = {chirp!r}: None, True or an int of at least 7 (the smallest generic radix)')
    return int(chirp)


def route(n, chirp=None):
    """how a transform of length n runs under `chirp=` (host only): 'plain' -- built radices only; 'dense' -- its plan holds a generic radix
    (a thread per output over the r inputs; a prime length is the dense DFT); 'chirp' -- its plan holds a generic radix >= r0 and
    n <= 1 << 24: the whole length by the chirp route"""
    r0 = _chirp_r0(chirp)
    generic = [r for r in plan(n) if r not in BUILT_RADICES]
    if not generic:
        return 'plain'
    return 'chirp' if r0 is not None and max(generic) >= r0 and n <= MAX_CHIRP else 'dense'


def _check_length(n, chirp=None):
    if route(n, chirp) == 'chirp':
        return
    wide = [r for r in plan(n) if r not in BUILT_RADICES and r > MAX_GENERIC]
    if wide and _chirp_r0(chirp) is None:
        raise ValueError(f'a record of {n} samples has the prime factor {wide[0]}: above {MAX_GENERIC} its dense pass is not run (chirp= runs such a length)')
    if wide:
        raise ValueError(f'a record of {n} samples has the prime factor {wide[0]}: above {MAX_GENERIC} its dense pass is not run, and the chirp route '
                         f'takes at most 1 << 24 = {MAX_CHIRP} samples')


def twiddles(n, sign):
    """exp(sign * 2 pi i k / n), k < n, as an (n, 2) float64 array: the table `ecgvit_resample` takes for a length (sign -1: forward, +1: inverse)"""
    ang = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    return np.ascontiguousarray(np.stack([np.cos(ang), sign * np.sin(ang)], axis=-1))


def chirp_table(n, sign):
    """the chirp w[j] = exp(sign * i pi j^2 / n), j < n, as an (n, 2) float64 array: cos / sin(pi ((j j) mod 2 n) / n), the square and the
    reduction in 64-bit integers (j < 1 << 24)"""
    j = np.arange(n, dtype=np.int64)
    ang = np.pi * ((j * j) % (2 * n)).astype(np.float64) / n
    return np.ascontiguousarray(np.stack([np.cos(ang), sign * np.sin(ang)], axis=-1))


def _side_tables(n, sign, chirp, tables, device):
    """the device tables one side of `ecgvit_resample_chirp` takes -> (twiddles, chirp table, filter); plain: the table of (n, sign) and two
    None.  tables: the per-call cache, {(length, sign): twiddles, ('chirp', n, sign): w, ('filter', n, sign): DFT_M(b) / M}; the table of M is
    the forward table of that length, (M, -1), whatever the sign."""
    key = (chirp_length(n), -1) if chirp else (n, sign)
    if key not in tables:
        tables[key] = torch.from_numpy(twiddles(*key)).to(device)
    if not chirp:
        return tables[key], None, None
    M = key[0]
    if ('filter', n, sign) not in tables:
        w = tables[('chirp', n, sign)] = torch.from_numpy(chirp_table(n, sign)).to(device)
        filt = torch.empty((M, 2), dtype=torch.float64, device=device)
        ws = torch.empty((2 * M, 2), dtype=torch.float64, device=device)
        run.ecgvit_resample_chirp_filter(ptr(w), n, M, ptr(tables[key]), ptr(filt), ptr(ws), stream())
        tables[('filter', n, sign)] = filt
    return tables[key], tables[('chirp', n, sign)], tables[('filter', n, sign)]


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


def _run(x, src_off, lens, s_stride, out, dst_off, out_lens, d_stride, ws_bytes, tables, chirp=None):
    """resample the records (src_off, lens) of the device store x into (dst_off, out_lens) of the device store out: grouped by length, then by
    workspace.  tables: {(n, sign): device table} and the chirp route's entries (`_side_tables`), kept over the chunks of one call."""
    pairs = np.stack([lens, out_lens], axis=1)
    for n_in, n_out in np.unique(pairs, axis=0).tolist():
        g = np.nonzero((lens == n_in) & (out_lens == n_out))[0]
        src, dst = np.ascontiguousarray(src_off[g]), np.ascontiguousarray(dst_off[g])
        if n_in == n_out:
            _copy_records(x, out, src, s_stride, dst, d_stride, n_in)
            continue
        c_in, c_out = route(n_in, chirp) == 'chirp', route(n_out, chirp) == 'chirp'
        if c_in or c_out:
            need = lib().ecgvit_resample_chirp_workspace(1, C, n_in, n_out, c_in, c_out)
        else:
            need = lib().ecgvit_resample_workspace(1, C, n_in, n_out)
        step = min(ws_bytes // need, _MAX_GROUP, len(g))
        if step < 1:
            raise ValueError(f'workspace_bytes = {ws_bytes}: one record of {n_in} -> {n_out} samples needs {need}')
        tw_in, w_in, f_in = _side_tables(n_in, -1, c_in, tables, x.device)
        tw_out, w_out, f_out = _side_tables(n_out, 1, c_out, tables, x.device)
        ws = torch.empty(step * need // 8, dtype=torch.float64, device=x.device)
        src_d, dst_d = torch.from_numpy(src).to(x.device), torch.from_numpy(dst).to(x.device)
        for lo in range(0, len(g), step):
            cnt = min(step, len(g) - lo)
            if c_in or c_out:
                run.ecgvit_resample_chirp(ptr(x), ptr(out), ptr(src_d[lo:]), s_stride, ptr(dst_d[lo:]), d_stride, cnt, C, n_in, n_out,
                                          ptr(tw_in), ptr(tw_out), ptr(w_in), ptr(f_in), ptr(w_out), ptr(f_out), ptr(ws), stream())
            else:
                run.ecgvit_resample(ptr(x), ptr(out), ptr(src_d[lo:]), s_stride, ptr(dst_d[lo:]), d_stride, cnt, C, n_in, n_out,
                                    ptr(tw_in), ptr(tw_out), ptr(ws), stream())


def resample(records, fqs, fqs_target=250, num=None, offsets=None, idxs=None, chunk_records=None, workspace_bytes=None, chirp=None):
    """`scipy.signal.resample(lead, resampled_length(n, fqs, fqs_target))` for every lead of the selected records (f64 arithmetic, f32 loads and
    stores), into a new store: (R, 12, L') for a rectangle, ((12, S'), new_offsets) for a ragged store (new_offsets an int64 numpy table,
    the cumulative `resampled_length` in `idxs` order), a float32 numpy array (or pair) for a host array / memmap.
    fqs == fqs_target returns a bit-equal copy of the selected records, as wfdb does (no FFT round trip).
    num: the output length of a rectangle, instead of the rates' (a ragged store refuses it); num == L copies too.
    chunk_records: records per upload of a host store (None: about 256 MB of f32).
    workspace_bytes: the limit of the two complex f64 ping-pong buffers of a record group (None: 1 GiB; 32 bytes per sample and lead of the
    longer side, so a record of 462 600 samples needs 89 MB); more records run in several groups, and a single record that needs more raises
    with the number it needs.
    chirp: None -- today's routes, bits and refusals.  An int r0 >= 7: a length (before or after) whose plan holds a generic radix >= r0 is
    transformed whole by the chirp route (Bluestein, O(n log n); every other length keeps its plain passes, bit for bit); True: r0 =
    CHIRP_DEFAULT.  With chirp set a wide prime factor is refused only above 1 << 24 samples.  Per distinct length on the chirp route: one
    extra M-transform on the device (the filter spectrum) and two more table uploads, and 32 bytes per sample and lead of M =
    `resample_chirp_length(n)` instead of n in the workspace (the module's docstring).
    Launches: one sequence of 3 + passes(n_in) + passes(n_out) per distinct length and record group (the module's docstring says what a store
    of many distinct lengths costs); a chirp side runs 2 passes(M) + 1 instead of passes(n).  NaN samples are not supported."""
    _chirp_r0(chirp)
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
        _check_length(int(n), chirp)
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
            _run(records, s.src_off, lens, s.stride, out, dst_off, out_lens, d_stride, ws_bytes, tables, chirp)
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
            _run(x, np.asarray(off, np.int64), np.asarray(clens, np.int64), int(stride), o, dst_off, out_lens[first:first + cnt], d_stride, ws_bytes, tables, chirp)
            if s.rect:
                out[first:first + cnt] = o.cpu().numpy()
            else:
                out[:, new_off[first]:new_off[first + cnt]] = o.cpu().numpy()
            first += cnt
    return out if s.rect else (out, new_off)
