"""CPU: the masked pre-train objective over records of unequal length -- the mask sampler and the mask representation (flat record-local
indices + per-record counts), the token geometry of the two row layouts (engine.MaskedVarlenBatch), every refusal (raised from host tensors,
before anything could launch), the new C-ABI entry points, and the resources of the new kernels (code-object metadata; no GPU)."""
import inspect
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.engine import MaskedVarlenBatch, check_mask_varlen

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')
HEADER = os.path.join(ROOT, 'include', 'ecgvit_hip.h')
NEW_SYMBOLS = ('ecgvit_mask_embed_varlen_fwd', 'ecgvit_mask_embed_varlen_bwd')
L, P = 1000, 4
LENGTHS = torch.tensor([1000, 4, 400, 596])


def _model(dtype=torch.bfloat16, ratio=0.5, **kw):
    conf = E.EcgVitConfig(max_signal_length=L, patch_size=P, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    return E.MaskedEcgVit(E.EcgVit(num_class=7, config=conf, compute_dtype=dtype, **kw), mask_ratio=ratio)


# ------------------------------------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('ratio', [0.5, 0.15, 0.75])
def test_mask_counts(ratio):
    mm = _model(ratio=ratio)
    lengths = torch.tensor([1000, 4, 400, 596, 8, 12])
    c = mm.mask_counts(lengths)
    assert c.dtype == torch.int64 and not c.is_cuda and c.shape == (6,)
    assert c.tolist() == [max(1, int(ratio * (v // P))) for v in lengths.tolist()]
    assert int(c[0]) == mm.n_mask                      # a full-width record: today's count
    assert int(c[1]) == 1                              # a record of one patch masks it


def test_random_mask_indices_varlen():
    mm = _model()
    idx, counts = mm.random_mask_indices_varlen(LENGTHS, generator=torch.Generator().manual_seed(7))
    assert idx.dtype == torch.int32 and idx.dim() == 1 and not idx.is_cuda
    assert torch.equal(counts, mm.mask_counts(LENGTHS)) and idx.numel() == int(counts.sum())
    again, _ = mm.random_mask_indices_varlen(LENGTHS, generator=torch.Generator().manual_seed(7))
    other, _ = mm.random_mask_indices_varlen(LENGTHS, generator=torch.Generator().manual_seed(8))
    assert torch.equal(idx, again) and not torch.equal(idx, other)
    # the flat layout follows the counts: per record the head of one randperm(n_b) drawn from the generator, records in order
    g = torch.Generator().manual_seed(7)
    k = 0
    for nb, mb in zip((LENGTHS // P).tolist(), counts.tolist()):
        part = idx[k:k + mb]
        assert torch.equal(part, torch.randperm(nb, generator=g)[:mb].to(torch.int32))
        assert int(part.min()) >= 0 and int(part.max()) < nb and part.unique().numel() == mb
        k += mb


def test_rectangular_sampler_and_check_unchanged():
    mm = _model()
    idx = mm.random_mask_indices(3, generator=torch.Generator().manual_seed(1))
    assert idx.shape == (3, mm.n_mask) and idx.dtype == torch.int32
    g = torch.Generator().manual_seed(1)
    assert torch.equal(idx, torch.stack([torch.randperm(mm.n_patch, generator=g)[:mm.n_mask] for _ in range(3)]).to(torch.int32))
    mm.check_mask_indices(idx, 3)
    bad = idx.clone()
    bad[1, 0] = bad[1, 1]
    with pytest.raises(ValueError, match='duplicate'):
        mm.check_mask_indices(bad, 3)
    with pytest.raises(ValueError, match='lie in'):
        mm.check_mask_indices(torch.full((3, 2), 250, dtype=torch.int32), 3)
    assert list(inspect.signature(E.MaskedEcgVit.random_mask_indices).parameters) == ['self', 'batch', 'generator']
    assert list(inspect.signature(E.MaskedEcgVit.check_mask_indices).parameters) == ['self', 'mask_idx', 'batch']


def test_public_signatures():
    # forward takes lengths= / mask_counts= as keywords (and nothing else): they reach the validation, which answers before any device is needed
    mm = _model()
    idx, counts = mm.random_mask_indices_varlen(LENGTHS)
    with pytest.raises(ValueError, match='needs mask_counts'):
        mm(torch.zeros(4, 12, L), idx, lengths=LENGTHS)
    with pytest.raises(ValueError, match='needs lengths'):
        mm(torch.zeros(4, 12, L), idx, mask_counts=counts)
    with pytest.raises(TypeError, match='length'):
        mm(torch.zeros(4, 12, L), idx, length=LENGTHS)
    assert list(inspect.signature(E.HipTrainStep.step_masked).parameters) == ['self', 'sample_values', 'mask_idx', 'micro_batch_size', 'lengths',
                                                                               'mask_counts']


# ------------------------------------------------------------------------------------------------ geometry (hand-worked)
def test_geometry_packed_and_padded():
    # 250, 1, 100 and 149 patches; no CLS row anywhere
    idx = torch.tensor([3, 0, 249, 0, 99, 5, 148], dtype=torch.int64)
    counts = torch.tensor([3, 1, 2, 1])
    g = MaskedVarlenBatch(LENGTHS.to(torch.int64), P, torch.device('cpu')).set_mask(idx, counts)
    assert g.n_tok.tolist() == [250, 1, 100, 149] and g.tok_off.tolist() == [0, 250, 251, 351] and g.n_cls.tolist() == [251, 2, 101, 150]
    assert (g.M, g.N, g.S, g.B, g.m, g.n_pad) == (500, 250, 2000, 4, 7, 0)
    assert g.order.tolist() == [0, 3, 2, 1]
    assert g.rows.tolist() == [3, 0, 249, 250, 350, 256, 499] and g.rows.dtype == torch.int32
    p = MaskedVarlenBatch(LENGTHS.to(torch.int64), P, torch.device('cpu'), width=1000).set_mask(idx, counts)
    assert p.tok_off.tolist() == [0, 250, 500, 750] and (p.M, p.N, p.n_pad) == (1000, 250, 250)
    assert p.rows.tolist() == [3, 0, 249, 250, 599, 505, 898]
    # record range 1 .. 2: samples 1000 .. 1404, its own offsets and indices
    (s0, s1), h = g.records(1, 3)
    assert (s0, s1) == (1000, 1404) and h.n_tok.tolist() == [1, 100] and h.tok_off.tolist() == [0, 1] and h.rows.tolist() == [0, 100, 6]
    assert h.counts.tolist() == [1, 2] and h.m == 3 and h.order.tolist() == [1, 0]
    # ties keep the record order (a fixed summation order)
    t = MaskedVarlenBatch(torch.tensor([8, 400, 8, 400]), P, torch.device('cpu'))
    assert t.order.tolist() == [1, 3, 0, 2]


def test_full_width_equal_counts_is_the_rectangular_pass():
    mm = _model()
    full = torch.full((3,), L)
    idx2 = mm.random_mask_indices(3, generator=torch.Generator().manual_seed(2))
    g = mm.check_varlen_input(torch.zeros(3, 12, L), idx2.flatten(), full, torch.full((3,), mm.n_mask))
    assert torch.equal(g.as_rectangular(L), idx2)
    g = mm.check_varlen_input(torch.zeros(3, 12, L), idx2.flatten()[:-1], full, torch.tensor([125, 125, 124]))
    assert g.as_rectangular(L) is None                       # unequal counts
    g = mm.check_varlen_input(torch.zeros(12, 3 * L), idx2.flatten(), full, torch.full((3,), mm.n_mask))
    assert g.as_rectangular(L) is None                       # a ragged batch stays packed


# ------------------------------------------------------------------------------------------------ refusals: ValueError from host tensors, no device
def _good(mm, lengths=LENGTHS):
    return mm.random_mask_indices_varlen(lengths, generator=torch.Generator().manual_seed(3))


X3 = torch.zeros(4, 12, L)
XR = torch.zeros(12, int(LENGTHS.sum()))


@pytest.mark.parametrize('form', ['padded', 'ragged'])
@pytest.mark.parametrize('case,why', [
    ('idx_2d', r'not \(B, m\)'), ('idx_float', 'integer'), ('counts_float', 'integer'), ('counts_shape', 'shape'), ('counts_zero', '1 <= m_b'),
    ('counts_above_n', '1 <= m_b'), ('sum_mismatch', 'sum to'), ('idx_negative', 'lie in'), ('idx_past_record', 'lie in'),
    ('duplicate', 'duplicate'), ('lengths_float', 'integer'), ('lengths_multiple', 'multiple'), ('lengths_zero', 'positive'),
    ('lengths_shape', 'shape'), ('no_counts', 'needs mask_counts'),
])
def test_bad_masks_and_lengths_raise_before_any_launch(form, case, why):
    mm = _model()
    idx, counts = _good(mm)
    lengths = LENGTHS.clone()
    if case == 'idx_2d':
        idx = mm.random_mask_indices(4)
    elif case == 'idx_float':
        idx = idx.float()
    elif case == 'counts_float':
        counts = counts.float()
    elif case == 'counts_shape':
        counts = counts[:3]
    elif case == 'counts_zero':
        counts = torch.tensor([126, 0, 50, 74])
    elif case == 'counts_above_n':
        counts, idx = torch.tensor([125, 2, 50, 74]), torch.cat([idx, idx[:1]])
    elif case == 'sum_mismatch':
        idx = idx[:-1]
    elif case == 'idx_negative':
        idx[0] = -1
    elif case == 'idx_past_record':
        idx[125] = 1          # record 1 holds one patch: only index 0 exists
    elif case == 'duplicate':
        idx[126] = idx[127]   # two entries of record 2
    elif case == 'lengths_float':
        lengths = lengths.float()
    elif case == 'lengths_multiple':
        lengths = torch.tensor([1000, 6, 398, 596])
    elif case == 'lengths_zero':
        lengths = torch.tensor([1000, 0, 404, 596])
    elif case == 'lengths_shape':
        lengths = lengths[None]
    elif case == 'no_counts':
        counts = None
    x = X3 if form == 'padded' else XR
    with pytest.raises(ValueError, match=why):
        mm(x, idx, lengths=lengths, mask_counts=counts)
    with pytest.raises(ValueError, match=why):
        E.HipTrainStep(mm, dict(n_step=10)).step_masked(x, idx, lengths=lengths, mask_counts=counts)


def test_form_refusals():
    mm = _model()
    idx, counts = _good(mm)
    step = E.HipTrainStep(mm, dict(n_step=10))
    for call in (mm, step.step_masked):
        with pytest.raises(ValueError, match='ragged.*needs lengths'):
            call(XR, idx)
        with pytest.raises(ValueError, match='ragged.*needs lengths'):
            call(XR, idx, mask_counts=counts)
        with pytest.raises(ValueError, match='needs lengths'):
            call(X3, idx, mask_counts=counts)
        with pytest.raises(ValueError, match='sum'):
            call(XR[:, :-4], idx, lengths=LENGTHS, mask_counts=counts)
        with pytest.raises(ValueError, match='exceed'):
            call(X3[:, :, :996].contiguous(), idx, lengths=LENGTHS, mask_counts=counts)
        with pytest.raises(ValueError, match='exceed'):
            call(torch.zeros(12, 2004), idx, lengths=torch.tensor([1004, 4, 400, 596]), mask_counts=counts)
    m32 = _model(dtype=torch.float32)
    with pytest.raises(ValueError, match='bf16'):
        m32(XR, idx, lengths=LENGTHS, mask_counts=counts)
    with pytest.raises(RuntimeError, match='MI355X'):       # the padded form is legal on the f32 engine: only the device is missing here
        if torch.cuda.is_available():
            raise RuntimeError('MI355X')
        m32(X3, idx, lengths=LENGTHS, mask_counts=counts)
    conf = E.EcgVitConfig(max_signal_length=L, patch_size=P, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, intermediate_size=512,
                          hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    mf = E.MaskedEcgVit(E.EcgVit(num_class=7, config=conf, compute_dtype=torch.bfloat16, fp8_linear=True))
    for x, word in ((X3, 'lengths'), (XR, 'ragged')):
        with pytest.raises(ValueError, match=f'{word}.*fp8_linear'):
            mf(x, idx, lengths=LENGTHS, mask_counts=counts)
        with pytest.raises(ValueError, match=f'{word}.*fp8_linear'):
            E.HipTrainStep(mf, dict(n_step=10)).step_masked(x, idx, lengths=LENGTHS, mask_counts=counts)
    mt = _model()
    mt.encoder.set_input_transform(E.transform.FusedInputTransform([0.0] * 12, [1.0] * 12, P))
    for x, word in ((X3, 'lengths'), (XR, 'ragged')):
        with pytest.raises(ValueError, match=f'{word}.*input transform'):
            mt(x, idx, lengths=LENGTHS, mask_counts=counts)


def test_check_mask_varlen_accepts_what_the_sampler_draws():
    mm = _model()
    for seed in range(3):
        lengths = torch.randint(1, 251, (9,), generator=torch.Generator().manual_seed(seed)) * P
        idx, counts = mm.random_mask_indices_varlen(lengths, generator=torch.Generator().manual_seed(seed))
        i, c = check_mask_varlen(idx, counts, lengths // P)
        assert i.dtype == torch.int64 and torch.equal(i, idx.long()) and torch.equal(c, counts)


# ------------------------------------------------------------------------------------------------ C-ABI and code objects
def test_new_entry_points_declared_bound_and_exported():
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name
        assert name in hip.SIGNATURES
    assert hip.ABI_VERSION == 6
    if os.path.exists(LIB):
        import ctypes
        l = ctypes.CDLL(LIB)
        for name in NEW_SYMBOLS:
            getattr(l, name)
        assert l.ecgvit_abi_version() == 6
    tools_header = open(os.path.join(ROOT, 'tools', 'ecgvit_hip_tools.h')).read()
    assert not any(name in tools_header for name in NEW_SYMBOLS)


def test_new_kernels_spill_free():
    import code_objects
    if not os.path.exists(code_objects.READELF) or not os.path.exists(LIB):
        pytest.skip('needs the built library and llvm-readelf')
    ks = code_objects.kernels(LIB)
    for stem, n in (('mask_embed_varlen_kernel', 2), ('mask_embed_varlen_bwd_kernel', 2), ('mark_rows_kernel', 1)):
        hit = [k for name, k in ks.items() if stem in name]
        assert len(hit) == n, (stem, len(hit))
        for k in hit:
            assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (stem, k)
