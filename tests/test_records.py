"""CPU: the record-store convention of `records.py` -- the selection tables on their named fields, the gather of a host store into compact
float32 chunks and the scatter back -- and the denoiser resolving a selection once per public call."""
import numpy as np
import pytest
import torch

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import denoise, records as R


def test_selection_tables():
    x = np.zeros((4, 12, 30), np.float32)
    rag, off = np.zeros((12, 50), np.float32), np.array([0, 20, 50])
    s = R.select_records(rag, off, np.array([1, 0]))
    assert s.src_off.tolist() == [20, 0] and s.raw_len.tolist() == [30, 20] and s.stride == 50
    assert (s.rect, s.n, s.C, s.R, s.min_len, s.max_len, s.sel.tolist()) == (False, 2, 12, 2, 20, 30, [1, 0])
    s = R.select_records(x, None, np.array([3, 1]))
    assert s.src_off.tolist() == [3 * 360, 360] and s.raw_len.tolist() == [30, 30] and s.stride == 30
    assert (s.rect, s.n, s.C, s.R, s.min_len, s.max_len, s.sel.tolist()) == (True, 4, 12, 2, 30, 30, [3, 1])


def test_repeats_are_refused_only_on_request():
    x = np.zeros((4, 12, 30), np.float32)
    assert R.select_records(x, None, [1, 1, 2]).sel.tolist() == [1, 1, 2]          # the fit and the tokenizer read a record twice
    with pytest.raises(ValueError, match='repeats'):
        R.select_records(x, None, [1, 1, 2], unique=True)


def roundtrip(host, offsets, idxs, chunk_records, records_of):
    """every property of `host_chunks` over one store; records_of(store, i): record i as (12, l)"""
    s = R.select_records(host, offsets, idxs)
    out = host.copy()
    seen = []
    for buf, off, lens, stride, scatter in R.host_chunks(host, s, chunk_records):
        assert buf.dtype == np.float32 and buf.flags.c_contiguous and off.dtype == np.int64
        flat = buf.reshape(-1)
        for o, l in zip(off.tolist(), lens.tolist()):                       # off, lens and stride address the chunk as the kernels do
            i = s.sel[len(seen)]
            got = np.stack([flat[o + c * stride:o + c * stride + l] for c in range(12)])
            assert np.array_equal(got, records_of(host, i).astype(np.float32)) and l == records_of(host, i).shape[1]
            seen.append(int(i))
        assert len(lens) <= (chunk_records or len(s.sel))
        scatter(out, buf * 2)
    assert seen == list(idxs)
    for i in range(s.n):
        rec = records_of(host, i)
        want = (rec.astype(np.float32) * 2).astype(host.dtype) if i in idxs else rec             # doubled, or its own bits
        assert np.ascontiguousarray(records_of(out, i)).tobytes() == np.ascontiguousarray(want).tobytes(), i
    return len(seen)


@pytest.mark.parametrize('chunk_records', [1, 2, None])
def test_host_chunks_of_a_rectangle(chunk_records):
    host = np.random.default_rng(3).standard_normal((5, 12, 7))                # float64: rounded once, on the way into the chunk
    roundtrip(host, None, [4, 1, 2], chunk_records, lambda a, i: a[i])


def test_host_chunks_of_a_ragged_store():
    off = np.concatenate([[0], np.cumsum([3, 7, 1, 5])])
    host = np.random.default_rng(4).standard_normal((12, 16)).astype(np.float32)
    roundtrip(host, off, [3, 0], 1, lambda a, i: a[:, off[i]:off[i + 1]])


def test_chunk_size():
    s = R.select_records(np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (3, 12, 5000), (0, 0, 0)), None, None)
    assert R.chunk_step(s) == 64 * 2 ** 20 // (12 * 5000) and R.chunk_step(s, 7) == 7
    with pytest.raises(ValueError, match='chunk_records'):
        R.chunk_step(s, 0)
    with pytest.raises(ValueError, match='chunk_records'):                     # refused when the chunks are asked for, before the first is gathered
        R.host_chunks(np.zeros((3, 12, 8), np.float32), s, 0)


def test_the_denoiser_resolves_a_selection_once_per_call(monkeypatch):
    calls = []

    def counted(*a, **kw):
        calls.append(a)
        return R.select_records(*a, **kw)
    monkeypatch.setattr(denoise, 'select_records', counted)
    x = np.random.default_rng(5).standard_normal((3, 12, 64)).astype(np.float32)
    for fn in (lambda: E.lowpass(x), lambda: E.nlm(x, sigma=np.ones((2, 12)), idxs=[2, 0]), lambda: E.rloess(x, 31),
               lambda: E.EcgDenoiser(loess_points=31)(x, baseline='rloess')):
        del calls[:]
        if torch.cuda.is_available():
            fn()
        else:
            with pytest.raises(RuntimeError, match='no CPU fallback'):
                fn()
        assert len(calls) == 1
