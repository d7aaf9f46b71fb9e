"""CPU: fused input transforms for records of unequal raw length (`FusedInputTransform(per_record=True)`): the token and raw geometry of the
padded, ragged and masked layouts from hand-written raw lengths, slicing by record range (raw offsets for the input, padded ones for the
token rows), the refusals that come before any launch, the per-record TimeOut draw against the reference's calls written out here, the new
C-ABI entry point and its kernels' resources (code-object metadata), and the ragged feeder on device='cpu'.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import abi_header

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.engine import (VitEngine, RaggedBatch, RawPaddedBatch, MaskedVarlenBatch, check_raw_lengths, ragged_slice,
                                                    check_masked_varlen_input)

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')
P, C = 4, 12
RAW = torch.tensor([1, 3, 8, 7, 30])     # l = 1, l < P, l = 2 P (the quirk: 3 patches), l = 2 P - 1, l = 7 P + 2
PADDED = [4, 4, 12, 8, 32]
N_PATCH = [1, 1, 3, 2, 8]


def _xf(per_record=True, **kw):
    return E.FusedInputTransform(mean=[0.0] * 12, std=[1.0] * 12, patch_size=P, per_record=per_record, **kw)


def _engine(dtype=torch.bfloat16, N=251, xf=None, **kw):
    eng = VitEngine(C=C, L=P * (N - 1), P=P, d=128, h=2, f=256, Ly=2, K=5, p_hidden=0.0, p_emb=0.0, dtype=dtype, layout=None, **kw)
    eng.input_transform = xf
    return eng


def test_padded_lengths_hand_worked():
    raw, padded = check_raw_lengths(RAW, _xf(), 1000)
    assert raw.tolist() == RAW.tolist() and padded.tolist() == PADDED
    assert [_xf().padded_length(int(l)) for l in RAW] == PADDED


def test_ragged_geometry_hand_worked():
    eng = _engine(xf=_xf())
    rg = eng.check_ragged_input(torch.zeros(C, 49), RAW, labels=torch.zeros(5, 5))
    assert rg.n_tok.tolist() == [n + 1 for n in N_PATCH]
    assert rg.tok_off.tolist() == [0, 2, 4, 8, 11]            # CLS rows: prefix sums of n_b + 1
    assert (rg.M, rg.N, rg.S, rg.S_raw, rg.B) == (20, 9, 60, 49, 5)
    rs = rg.rawside
    assert rs.src_off.dtype == torch.int64 and rs.src_off.tolist() == [0, 1, 4, 12, 19]     # raw offsets
    assert rs.raw_len.tolist() == RAW.tolist() and rs.n_patch.tolist() == N_PATCH
    assert rs.row_off.tolist() == [0, 1, 2, 5, 7]             # patch rows carry no CLS row: padded offsets / P
    assert (rs.lead_stride, rs.nrows, rs.n_max) == (49, 0, 8)
    assert eng.check_ragged_input(torch.zeros(C, 49), rg) is rg
    with pytest.raises(ValueError, match='RaggedBatch'):
        eng.check_ragged_input(torch.zeros(C, 60), rg)        # S_raw, not the padded S, is the batch's width
    with pytest.raises(ValueError, match='RaggedBatch'):
        _engine().check_ragged_input(torch.zeros(C, 49), rg)  # a raw geometry on an engine without the transform


def test_ragged_slices_cut_input_by_raw_and_rows_by_padded_offsets():
    x = torch.arange(C * 49, dtype=torch.float32).view(C, 49)
    recs = torch.split(x, RAW.tolist(), dim=1)
    rg = _engine(xf=_xf()).check_ragged_input(x, RAW)
    for b0, b1 in ((0, 2), (2, 5), (1, 4), (0, 5)):
        xs, part = ragged_slice(x, rg, b0, b1)
        assert torch.equal(xs, torch.cat(recs[b0:b1], dim=1))
        want = RaggedBatch(torch.tensor(PADDED[b0:b1]), P, x.device, RAW[b0:b1])
        assert part.n_tok.tolist() == want.n_tok.tolist() and part.tok_off.tolist() == want.tok_off.tolist()
        assert part.rawside.src_off.tolist() == want.rawside.src_off.tolist() and part.rawside.src_off[0] == 0
        assert part.rawside.row_off.tolist() == want.rawside.row_off.tolist()
        assert (part.S_raw, part.S, part.M) == (xs.shape[1], sum(PADDED[b0:b1]), sum(N_PATCH[b0:b1]) + b1 - b0)
        assert part.rawside.lead_stride == xs.shape[1]
        xs2, ls = ragged_slice(x, RAW, b0, b1)                # a plain tensor of raw lengths cuts at the raw offsets too
        assert torch.equal(xs2, xs) and ls.tolist() == RAW[b0:b1].tolist()


def test_padded_form_geometry_and_slices():
    eng = _engine(xf=_xf())
    W = 33                                                    # any W >= max l_b, no multiple-of-P rule
    rp = eng.check_raw_input(torch.zeros(5, C, W), RAW)
    assert isinstance(rp, RawPaddedBatch) and rp.width == 32 and rp.ntok.tolist() == [n + 1 for n in N_PATCH]
    rs = rp.rawside
    assert rs.src_off.tolist() == [b * C * W for b in range(5)] and rs.row_off.tolist() == [b * 8 for b in range(5)]
    assert (rs.lead_stride, rs.nrows, rs.n_max) == (W, 8, 8) and rs.n_patch.tolist() == N_PATCH
    part = rp.records(1, 4)                                   # a micro-batch keeps the whole batch's pass width
    assert part.width == 32 and part.ntok.tolist() == [2, 4, 3] and part.rawside.nrows == 8
    assert part.rawside.src_off.tolist() == [0, C * W, 2 * C * W] and part.rawside.row_off.tolist() == [0, 8, 16]
    assert eng.check_raw_input(torch.zeros(5, C, W), rp) is rp
    full = eng.check_raw_input(torch.zeros(3, C, 999), None)  # no lengths: every record holds W samples
    assert full.raw.tolist() == [999] * 3 and full.width == 1000 and full.ntok is None    # all fill the width: the uniform kernels


@pytest.mark.parametrize('ragged', [False, True])
def test_masked_geometry_and_slices(ragged):
    xf = _xf()
    x = torch.zeros(C, 49) if ragged else torch.zeros(5, C, 33)
    counts = torch.tensor([1, 1, 2, 1, 3])
    idx = torch.tensor([0, 0, 2, 0, 1, 7, 0, 3])
    kw = dict(C=C, P=P, max_len=1000, dtype=torch.bfloat16, fp8=False, input_transform=xf)
    geo = check_masked_varlen_input(x, idx, RAW, counts, **kw)
    assert isinstance(geo, MaskedVarlenBatch) and geo.n_tok.tolist() == N_PATCH and geo.N == 8 and geo.as_rectangular(1000) is None
    if ragged:
        assert geo.tok_off.tolist() == [0, 1, 2, 5, 7] and geo.M == 15 and geo.n_pad == 0
        assert geo.rawside.src_off.tolist() == [0, 1, 4, 12, 19] and (geo.rawside.lead_stride, geo.rawside.nrows) == (49, 0)
        assert geo.rows.tolist() == [0, 1, 4, 2, 6, 14, 7, 10]      # tok_off[b] + the record-local index
    else:
        assert geo.tok_off.tolist() == [0, 8, 16, 24, 32] and geo.M == 40 and geo.n_pad == 8 and geo.width == 32
        assert geo.rawside.src_off.tolist() == [b * C * 33 for b in range(5)] and (geo.rawside.lead_stride, geo.rawside.nrows) == (33, 8)
    assert geo.rawside.row_off.tolist() == geo.tok_off.tolist() and geo.rawside.raw_len.tolist() == RAW.tolist()
    (s0, s1), part = geo.records(2, 5)
    assert (s0, s1) == (4, 49)                                # RAW offsets
    assert part.n_tok.tolist() == [3, 2, 8] and part.m == 6 and part.idx_host.tolist() == [2, 0, 1, 7, 0, 3]
    if ragged:
        assert part.rawside.src_off.tolist() == [0, 8, 15] and part.rawside.lead_stride == 45 and part.tok_off.tolist() == [0, 3, 5]
    else:
        assert part.rawside.src_off.tolist() == [0, C * 33, 2 * C * 33] and part.n_pad == 8 and part.tok_off.tolist() == [0, 8, 16]
    with pytest.raises(ValueError, match='n_b'):              # counts are checked against padded_length(l_b) / P patches
        check_masked_varlen_input(x, torch.tensor([0, 1, 0, 0, 0]), RAW, torch.tensor([2, 1, 1, 1, 1]), **kw)


def test_mask_helpers_take_raw_lengths_under_a_per_record_transform():
    conf = E.EcgVitConfig(max_signal_length=1000, patch_size=P, hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256)
    mm = E.MaskedEcgVit(E.EcgVit(num_class=3, config=conf, compute_dtype=torch.bfloat16), mask_ratio=0.5)
    assert mm.patch_counts(torch.tensor(PADDED)).tolist() == N_PATCH                  # no transform: lengths / P
    assert mm.patch_counts(RAW, raw=True).tolist() == N_PATCH
    mm.encoder.set_input_transform(_xf())
    assert mm.patch_counts(RAW).tolist() == N_PATCH and mm.mask_counts(RAW).tolist() == [1, 1, 1, 1, 4]
    idx, counts = mm.random_mask_indices_varlen(RAW, generator=torch.Generator().manual_seed(0))
    assert counts.tolist() == [1, 1, 1, 1, 4] and idx.numel() == 8 and int(idx[-4:].max()) < 8
    geo = mm.check_varlen_input(torch.zeros(C, 49), idx, RAW, counts)
    assert geo.rawside is not None and geo.m == 8


@pytest.mark.parametrize('bad,why', [
    (torch.tensor([1.0, 3.0]), 'integer'), (torch.tensor([True, True]), 'integer'), (torch.tensor([0, 8]), 'positive'),
    (torch.tensor([-1, 8]), 'positive'), (torch.tensor([[4, 8]]), 'shape'), ([4, 8], 'tensor'), (torch.tensor([4, 1000]), 'max_signal_length'),
])
def test_invalid_raw_lengths_are_rejected(bad, why):
    with pytest.raises(ValueError, match=why):
        check_raw_lengths(bad, _xf(), 1000)


def test_refusals_before_any_launch():
    eng = _engine(xf=_xf())
    with pytest.raises(ValueError, match='exceed'):           # l > W
        eng.forward(torch.zeros(2, C, 30), lengths=torch.tensor([31, 4]))
    with pytest.raises(ValueError, match='shape'):
        eng.forward(torch.zeros(2, C, 30), lengths=torch.tensor([30]))
    with pytest.raises(ValueError, match='sum'):              # sum != S_raw
        eng.forward(torch.zeros(C, 49), lengths=torch.tensor([1, 3, 8, 7, 29]))
    with pytest.raises(ValueError, match='needs lengths'):
        eng.forward(torch.zeros(C, 49))
    with pytest.raises(ValueError, match='max_signal_length'):   # n_b over the maximum: 1000 raw samples pad to 1004
        eng.forward(torch.zeros(1, C, 1000), lengths=torch.tensor([1000]))
    with pytest.raises(ValueError, match='max_signal_length'):
        eng.forward(torch.zeros(C, 1000), lengths=torch.tensor([1000]))
    with pytest.raises(ValueError, match='bf16'):             # the ragged form on the f32 engine
        _engine(torch.float32, xf=_xf()).forward(torch.zeros(C, 49), lengths=RAW)
    f8 = VitEngine(C=C, L=1000, P=P, d=256, h=4, f=512, Ly=2, K=5, p_hidden=0.0, p_emb=0.0, dtype=torch.bfloat16, layout=None, fp8_linear=True)
    f8.input_transform = _xf()
    with pytest.raises(ValueError, match='fp8_linear'):
        f8.forward(torch.zeros(C, 49), lengths=RAW)
    with pytest.raises(ValueError, match='fp8_linear'):
        f8.forward(torch.zeros(5, C, 33), lengths=RAW)
    kw = dict(C=C, P=P, max_len=1000, input_transform=_xf())
    with pytest.raises(ValueError, match='fp8_linear'):
        check_masked_varlen_input(torch.zeros(C, 49), torch.zeros(5, dtype=torch.int64), RAW, torch.ones(5, dtype=torch.int64), dtype=torch.bfloat16, fp8=True, **kw)
    with pytest.raises(ValueError, match='bf16'):
        check_masked_varlen_input(torch.zeros(C, 49), torch.zeros(5, dtype=torch.int64), RAW, torch.ones(5, dtype=torch.int64), dtype=torch.float32, fp8=False, **kw)


def test_default_transform_still_refuses_lengths_and_ragged_batches():
    eng = _engine(xf=_xf(per_record=False))
    assert E.FusedInputTransform([0.0] * 12, [1.0] * 12, P).per_record is False
    with pytest.raises(ValueError, match='input transform'):
        eng.forward(torch.zeros(C, 600), lengths=torch.tensor([600]))
    eng.input_transform = _xf(per_record=False)
    with pytest.raises(ValueError, match='input transform'):
        eng.forward(torch.zeros(2, C, 996), lengths=torch.tensor([996, 400]))
    with pytest.raises(ValueError, match='input transform'):
        check_masked_varlen_input(torch.zeros(C, 8), torch.tensor([0]), torch.tensor([8]), torch.tensor([1]), C=C, P=P, max_len=1000,
                                  dtype=torch.bfloat16, fp8=False, input_transform=_xf(per_record=False))


# ------------------------------------------------------------------------------------------------ TimeOut
@pytest.mark.parametrize('seed', [0, 7])
def test_per_record_timeout_draw_is_the_references_calls_on_each_padded_length(seed):
    xf = _xf(timeout=True, timeout_scale=(0.0, 0.5))
    padded = [20, 5000, 4, 404, 1000, 32]
    torch.manual_seed(seed)
    got = xf.draw_timeout_records(padded)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 6)
    torch.manual_seed(seed)
    sampler = torch.distributions.Uniform(low=0.0, high=0.5)       # transform.py:178
    want = []
    for l in padded:                                               # transform.py:180-183, one record at a time
        r = sampler.sample()
        l_crop = round(float(r) * l)
        start = torch.randint(high=l - l_crop, size=(1,)).item()
        want.append((start, l_crop))
    assert got[0].tolist() == [s for s, _ in want] and got[1].tolist() == [c for _, c in want]
    assert all(0 <= s and s + c <= l for (s, c), l in zip(want, padded))
    # range by range, in order: the draw sequence of the unsplit batch
    torch.manual_seed(seed)
    parts = torch.cat([xf.draw_timeout_records(padded[a:b]) for a, b in ((0, 2), (2, 5), (5, 6))], dim=1)
    assert torch.equal(parts, got)


# ------------------------------------------------------------------------------------------------ ABI / code object
def test_entry_point_declared_bound_and_exported():
    name = 'ecgvit_patch_gather_transform_varlen'
    assert abi_header.held({name: 19}, hip.SIGNATURES)[name][0] == 'int'
    import ctypes
    assert hasattr(ctypes.CDLL(LIB), name)
    assert ctypes.CDLL(LIB).ecgvit_abi_version() == 6


def test_kernels_spill_free_no_scratch_lds_within_the_launchers_rule():
    import code_objects
    assert os.path.exists(code_objects.READELF), 'llvm-readelf is needed to read the code object'
    ks = {n: k for n, k in code_objects.kernels(LIB).items() if 'patch_gather_transform_varlen_kernel' in n}
    assert len(ks) == 2, sorted(ks)     # f32 and bf16 rows
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['group_segment_fixed_size'] == 0, (n, k)     # dynamic LDS only: the launcher sizes it, at most 48 KiB unless one patch needs more
    # the launcher's tile rule, restated: C (PB P + 1) floats with PB halved until it fits 48 KiB
    for p in (4, 20, 25, 500):
        pb = max(1, 256 // p)
        while pb > 1 and C * (pb * p + 1) * 4 > 48 * 1024:
            pb >>= 1
        assert C * (pb * p + 1) * 4 <= 48 * 1024


# ------------------------------------------------------------------------------------------------ feeder
def _store(n=11, seed=0):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, size=n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    store = rng.standard_normal((C, int(off[-1])))            # float64, as the reference's record files
    labels = (rng.random((n, 5)) < 0.3).astype(np.float32)
    return store, off, labels


def test_ragged_feeder_reproduces_the_records_in_order(tmp_path):
    store, off, labels = _store()
    idxs = np.array([9, 0, 4, 4, 10, 2, 7])
    for src, osrc in ((store, off), (str(tmp_path / 's.npy'), str(tmp_path / 'o.npy'))):
        if isinstance(src, str):
            np.save(src, store)
            np.save(osrc, off)
        f = E.RaggedDeviceFeeder(src, osrc, idxs, labels[idxs], batch_size=3, device='cpu')
        assert len(f) == 3
        seen = 0
        for batch in f:
            b = batch['labels'].shape[0]
            rows = idxs[seen:seen + b]
            want = np.concatenate([store[:, off[i]:off[i + 1]] for i in rows], axis=1).astype(np.float32)
            assert batch['sample_values'].dtype == torch.float32 and batch['sample_values'].is_contiguous()
            assert np.array_equal(batch['sample_values'].numpy(), want)
            assert batch['lengths'].dtype == torch.int64 and batch['lengths'].tolist() == [int(off[i + 1] - off[i]) for i in rows]
            assert np.array_equal(batch['labels'].numpy(), labels[rows])
            assert int(batch['lengths'].sum()) == batch['sample_values'].shape[1]
            seen += b
        assert seen == len(idxs)


def test_ragged_feeder_orders_shards_and_pads_as_device_feeder():
    store, off, labels = _store(n=10)
    idxs = np.arange(10)
    rect = np.zeros((10, C, 8))
    for kw in (dict(shuffle=True, seed=5), dict(rank=1, world=3), dict(rank=2, world=3, pad=False), dict(rank=0, world=4, drop_last=True),
               dict(shuffle=True, rank=1, world=2)):
        a = E.RaggedDeviceFeeder(store, off, idxs, labels, batch_size=2, device='cpu', **kw)
        b = E.DeviceFeeder(rect, idxs, labels, batch_size=2, device='cpu', **kw)
        for _ in range(2):      # two epochs: the shuffle moves on with the epoch in both
            assert len(a) == len(b) and a._order().tolist() == b._order().tolist()
            la = [x['labels'] for x in a]
            lb = [x['labels'] for x in b]
            assert len(la) == len(lb) and all(torch.equal(u, v) for u, v in zip(la, lb))
    with pytest.raises(ValueError, match='offsets'):
        E.RaggedDeviceFeeder(store, off[:-1], idxs, labels, batch_size=2, device='cpu')
    with pytest.raises(ValueError, match=r'\(C, S_total\)'):
        E.RaggedDeviceFeeder(rect, off, idxs, labels, batch_size=2, device='cpu')
