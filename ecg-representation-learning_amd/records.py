"""
The one record-store convention of the normalise fit (`transform.fit_dynamic_normalize`), the segment tokenizer (`tokenizer.EcgTokenizer`) and the
denoiser (`denoise`): records are an (n, 12, L) rectangle, or a ragged (12, S_total) store with `offsets` (the (n + 1,) table
`RaggedDeviceFeeder` takes), and `idxs` selects records of either without a copy.  Every kernel of `csrc/fit_stats.hip`, `csrc/tokenize.hip` and
`csrc/denoise.hip` addresses the selected records through the same tables: `src_off` (int64: where lead 0 of a record starts), `raw_len` (int32),
the lead stride and the record count R.

`select_records` validates a store and resolves the selection on the host (`RecordSelection`), `check_device_store` holds a device store to
float32 / device / contiguous, `DeviceTables` puts a selection's tables on the device beside their host copies, and `host_chunks` gathers a host
store into compact float32 chunks (numpy: the upload is the caller's line) and scatters them back.
"""
import numpy as np
import torch

_CHUNK_F32 = 64 * 2 ** 20   # samples per default chunk of a host store: about 256 MB of f32


class RecordSelection:
    """the selected records of one store, on the host: rect (an (n, 12, L) rectangle?), n records in the store, C leads, per selected record
    `src_off` (int64) and `raw_len` (int64), the lead `stride`, the record indices `sel`, and min_len, max_len, R over the selection"""

    def __init__(self, rect, n, C, src_off, raw_len, stride, sel):
        self.rect, self.n, self.C, self.src_off, self.raw_len, self.stride, self.sel = rect, n, C, src_off, raw_len, int(stride), sel
        self.R, self.min_len, self.max_len = len(sel), int(raw_len.min()), int(raw_len.max())


def select_records(records, offsets, idxs, unique=False):
    """-> RecordSelection.  records: anything with the `.shape` of a store.  unique: refuse an `idxs` that names a record twice (a writer's
    check: readers take repeats)."""
    shape = tuple(records.shape)
    if len(shape) == 3:
        if offsets is not None:
            raise ValueError('offsets come with a ragged (12, S_total) store, not with (n, 12, L) records')
        n, C, L = shape
        if L < 1 or L > 2 ** 31 - 1:
            raise ValueError(f'records of {L} samples')
        off_all, len_all, stride = np.arange(n, dtype=np.int64) * (C * L), np.full(n, L, np.int64), L
    elif len(shape) == 2:
        if offsets is None:
            raise ValueError('a ragged (12, S_total) store needs offsets, an (n + 1,) table')
        C, S = shape
        off = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets).astype(np.int64)
        if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != S or (np.diff(off) <= 0).any():
            raise ValueError('offsets must be (n + 1,) strictly increasing from 0 to S_total')
        if int(np.diff(off).max()) > 2 ** 31 - 1:
            raise ValueError('a record is longer than 2^31 - 1 samples')
        n, off_all, len_all, stride = len(off) - 1, off[:-1], np.diff(off), S
    else:
        raise ValueError(f'records must be (n, 12, L) or a ragged (12, S_total) store with offsets, got shape {shape}')
    if C != 12:
        raise ValueError(f'records must hold 12 leads, got {C}')   # transform.py:26
    if idxs is None:
        sel = np.arange(n, dtype=np.int64)
    else:
        sel = np.asarray(idxs.cpu() if isinstance(idxs, torch.Tensor) else idxs)
        if sel.dtype == bool or sel.ndim != 1 or not np.issubdtype(sel.dtype, np.integer):
            raise ValueError('idxs must be a 1-D integer array of record indices')
        sel = sel.astype(np.int64)
        if len(sel) and (sel.min() < 0 or sel.max() >= n):
            raise ValueError(f'idxs out of range for {n} records')
    if len(sel) == 0:
        raise ValueError('no record selected')
    if unique and len(np.unique(sel)) != len(sel):
        raise ValueError('idxs repeats a record: two workgroups would write the same samples')
    return RecordSelection(len(shape) == 3, n, C, off_all[sel], len_all[sel], stride, sel)


def check_device_store(x, what='records'):
    """a store the kernels read in place: a contiguous float32 device tensor"""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise ValueError(f'{what} must be a float32 device tensor (no CPU fallback exists; a host tensor is taken as a host array only where one is)')
    if x.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {x.dtype}')
    if not x.is_contiguous():
        raise ValueError(f'{what} must be contiguous')


class DeviceTables:
    """the device tables of the runs of one device store `x`: `src_off` (int64) and `raw_len` (int32) on x's device, their host copies
    `src_off_h` / `raw_len_h` (int64), the lead `stride`, and R, min_len, max_len"""

    def __init__(self, x, src_off, raw_len, stride):
        self.x, self.R, self.stride = x, len(raw_len), int(stride)
        self.src_off_h, self.raw_len_h = np.ascontiguousarray(src_off, np.int64), np.ascontiguousarray(raw_len, np.int64)
        self.src_off = torch.from_numpy(self.src_off_h.copy()).to(x.device)
        self.raw_len = torch.from_numpy(self.raw_len_h.astype(np.int32)).to(x.device)
        self.min_len, self.max_len = int(self.raw_len_h.min()), int(self.raw_len_h.max())

    @classmethod
    def of(cls, x, s):
        """the tables of the selection `s` of the device store `x`"""
        return cls(x, s.src_off, s.raw_len, s.stride)


def chunk_step(s, chunk_records=None):
    """records per chunk of a host store: `chunk_records`, at least 1; None: about 256 MB of f32"""
    if chunk_records is None:
        return max(1, int(_CHUNK_F32 // (s.C * max(1, s.max_len))))
    if int(chunk_records) < 1:
        raise ValueError('chunk_records must be at least 1')
    return int(chunk_records)


def host_chunks(host, s, chunk_records=None):
    """-> per chunk (buffer, off, lens, stride, scatter): the records of the selection `s` of the host store `host` (an array / memmap of any float
    type), `chunk_records` at a time and in `idxs` order, as a compact float32 numpy store of the same form -- a (k, 12, L) rectangle or a
    ragged (12, S) -- with the src_off, raw_len and lead stride that address it; scatter(host_out, array) writes an array of the buffer's shape
    back where the chunk's records came from.  `chunk_records` is checked here, before the first chunk is asked for."""
    step = chunk_step(s, chunk_records)

    def chunks():
        for lo in range(0, s.R, step):
            ids, lens, srcs = s.sel[lo:lo + step], s.raw_len[lo:lo + step], s.src_off[lo:lo + step]
            if s.rect:
                L = int(lens[0])
                buf = np.ascontiguousarray(host[ids], dtype=np.float32)   # (k, C, L)
                off, stride = np.arange(len(ids), dtype=np.int64) * (s.C * L), L

                def scatter(host_out, arr, ids=ids):
                    host_out[ids] = arr
            else:
                S = int(lens.sum())
                buf = np.empty((s.C, S), np.float32)
                off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
                runs = list(zip(off.tolist(), srcs.tolist(), lens.tolist()))
                for o, src, l in runs:
                    buf[:, o:o + l] = host[:, src:src + l]      # (float64 -> float32 happens in this assignment, as in the feeders)
                stride = S

                def scatter(host_out, arr, runs=runs):
                    for o, src, l in runs:
                        host_out[:, src:src + l] = arr[:, o:o + l]
            yield buf, off, lens, stride, scatter
    return chunks()
