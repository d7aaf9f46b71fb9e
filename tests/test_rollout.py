"""CPU: attention rollout for whole batches -- the closed form the kernels implement agrees with the reference's loop, the `ecgvit_rollout_*`
entry points are declared, exported and bound without an ABI bump, their argument checks run on the host, and `attention_rollout_batch` /
`HipRollout` / `attention_rollout_saved` refuse bad arguments before any device work (no GPU)."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_micro
import abi_header

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.engine import VitEngine
from rollout_ref import rollout_reference, rollout_closed_form, rollout_closed_form_qkv, lse_from_qkv, probs_from_qkv

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')
P = 4
NEW = {'ecgvit_rollout_workspace': 3, 'ecgvit_rollout_cls': 13, 'ecgvit_rollout_colsum': 15, 'ecgvit_rollout_finish': 6}


def _softmax_layers(layers, h, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(3.0 * torch.randn(layers, h, n, n, generator=g), dim=-1)   # f32 rows: their sums are 1 up to rounding


@pytest.mark.parametrize('n,layers', [(2, 2), (3, 3), (251, 3)])
def test_closed_form_is_the_reference_loop_synthetic(n, layers):
    p = _softmax_layers(layers, 2, n, seed=n)
    a, b = rollout_reference(p), rollout_closed_form(p)
    assert a.shape == b.shape == (layers, n - 1)
    assert float((a - b).abs().max()) < 1e-6
    assert float(b.max()) == 1.0 and float(b.min()) >= 0.0


@pytest.mark.parametrize('tag', ['g2560', 't128'])
def test_closed_form_is_the_reference_loop_on_golden_probabilities(tag):
    z, _ = load_micro(tag)
    keys = sorted(k for k in z.files if re.fullmatch(r'inter/l\d+/probs', k))
    assert keys, 'the fixture holds no attention probabilities'
    per_layer = [torch.from_numpy(np.asarray(z[k])) for k in keys]       # each (B, h, n, n)
    B = per_layer[0].shape[0]
    for b in range(B):
        p = torch.stack([l[b] for l in per_layer])
        assert float((rollout_reference(p) - rollout_closed_form(p)).abs().max()) < 1e-6
    if B > 1:   # two different records' probabilities as two layers: the layer-pair product on fixture data
        p = torch.stack([per_layer[0][0], per_layer[0][1], per_layer[0][0]])
        assert float((rollout_reference(p) - rollout_closed_form(p)).abs().max()) < 1e-6


def test_closed_form_from_qkv_rebuilds_the_probabilities():
    g = torch.Generator().manual_seed(5)
    h, dh, n = 2, 8, 9
    qkvs = [torch.randn(n, 3 * h * dh, generator=g) for _ in range(3)]
    lses = [lse_from_qkv(q, h, dh, dh ** -0.5) for q in qkvs]
    p = torch.stack([probs_from_qkv(q, l, h, dh, dh ** -0.5) for q, l in zip(qkvs, lses)])
    assert float((p.sum(-1) - 1).abs().max()) < 1e-12
    assert float((rollout_closed_form_qkv(qkvs, lses, h, dh, dh ** -0.5) - rollout_reference(p)).abs().max()) < 1e-12
    one = rollout_closed_form(torch.ones(2, 1, 1, 1))   # a record of one token: an empty map
    assert one.shape == (2, 0)


def test_entry_points_declared_exported_and_bound_at_abi_6():
    so = ctypes.CDLL(hip.LIB_PATH)
    decls = abi_header.held(NEW, hip.SIGNATURES)
    for name in NEW:
        assert decls[name][0] in ('int', 'int64_t') and hasattr(so, name)
    assert hip.ABI_VERSION == 6 and hip.lib().ecgvit_abi_version() == 6
    assert hip.lib().ecgvit_rollout_workspace(512, 251, 12) == 4 * 512 * 251 * 12
    assert hip.lib().ecgvit_rollout_workspace(0, 251, 12) == 0


def test_kernel_argument_checks_run_on_the_host():
    """every refusal returns ECGVIT_EINVAL before anything is launched (no pointer is dereferenced)"""
    l = hip.lib()
    q, s, p, w, r, ws, nt, to = (0x10000000 * i for i in range(1, 9))

    def cls(qkv=q, lse=s, probs=None, c=r, n_tok=None, tok_off=None, B=2, N=9, h=2, dh=64, dtype=hip.BF16):
        return l.ecgvit_rollout_cls(qkv, lse, probs, c, n_tok, tok_off, B, N, h, dh, 0.125, dtype, None)

    def col(qkv=q, lse=s, probs=None, w=w, r=r, ws=ws, n_tok=None, tok_off=None, B=2, N=9, h=2, dh=64, dtype=hip.BF16):
        return l.ecgvit_rollout_colsum(qkv, lse, probs, w, r, ws, n_tok, tok_off, B, N, h, dh, 0.125, dtype, None)
    f32 = dict(qkv=None, lse=None, probs=p, dtype=hip.F32)
    for fn in (cls, col):
        assert fn(qkv=None) == 1 and fn(lse=None) == 1 and fn(probs=p) == 1           # bf16: qkv and lse, no probs
        assert fn(dh=32) == 1 and fn(dh=96) == 1 and fn(N=2049) == 1
        assert fn(B=0) == 1 and fn(N=0) == 1 and fn(h=0) == 1
        assert fn(tok_off=to) == 1                                                    # packed rows need the token counts
        assert fn(dtype=hip.FP8_E4M3) == 1 and fn(dtype=7) == 1
        assert fn(**{**f32, 'probs': None}) == 1 and fn(**{**f32, 'qkv': q}) == 1 and fn(**{**f32, 'lse': s}) == 1
        assert fn(**f32, n_tok=nt, tok_off=to) == 1                                   # f32: no packed rows
    assert cls(c=None) == 1 and col(w=None) == 1 and col(r=None) == 1 and col(ws=None) == 1
    fin = l.ecgvit_rollout_finish
    assert fin(None, None, 2, 3, 9, None) == 1 and fin(r, None, 0, 3, 9, None) == 1 and fin(r, None, 2, 0, 9, None) == 1 and fin(r, None, 2, 3, 0, None) == 1
    assert fin(r, None, 2, 3, 1, None) == 0   # one token per record: no patch column, nothing to launch


def _engine(dtype=torch.bfloat16, N=251, **kw):
    return VitEngine(C=12, L=P * (N - 1), P=P, d=128, h=2, f=256, Ly=2, K=5, p_hidden=0.0, p_emb=0.0, dtype=dtype, layout=None, **kw)


def test_rollout_saved_needs_a_full_supervised_forward():
    eng = _engine()
    with pytest.raises(RuntimeError, match='supervised forward'):
        eng.attention_rollout_saved()
    eng.saved = dict(B=2, masked=True)
    with pytest.raises(RuntimeError, match='masked objective'):
        eng.attention_rollout_saved()
    eng.saved = dict(B=2, masked=False, cls_only_last=True, ragged=None, ntok=None)
    with pytest.raises(RuntimeError, match='cls_only_last'):
        eng.attention_rollout_saved()


def test_bad_arguments_raise_before_any_device_work():
    model = E.EcgVit()
    with pytest.raises(ValueError, match='sample_values'):
        model.attention_rollout_batch(torch.zeros(2, 1, 12, 2560))
    with pytest.raises(ValueError, match='sample_values'):
        model.attention_rollout_batch(torch.zeros(2560))
    with pytest.raises(RuntimeError, match='MI355X'):
        model.attention_rollout_batch(torch.zeros(2, 12, 2560))
    with pytest.raises(RuntimeError, match='MI355X'):
        model.attention_rollout_batch(torch.zeros(12, 2560), lengths=torch.tensor([2560]))
    with pytest.raises(ValueError, match='batch_size'):
        E.HipRollout(model, batch_size=0)
    with pytest.raises(ValueError, match='sample_values'):
        E.HipRollout(model).rollout(torch.zeros(2, 1, 12, 2560))
    assert model.training   # left as it was


def test_public_surface():
    sig = inspect.signature(E.EcgVit.attention_rollout_batch).parameters
    assert list(sig) == ['self', 'sample_values', 'lengths'] and sig['lengths'].default is None
    assert E.RolloutOutput._fields == ('logits', 'maps', 'patch_counts')
    assert inspect.signature(E.HipRollout.__init__).parameters['batch_size'].default == 64
    assert list(inspect.signature(E.HipRollout.rollout).parameters) == ['self', 'sample_values', 'lengths']
    assert list(inspect.signature(E.EcgVit.attention_rollout).parameters) == ['self', 'sample_values']   # the one-record form is unchanged


def test_rollout_kernels_spill_free():
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    ks = {n: k for n, k in code_objects.kernels(LIB).items() if 'rollout_' in n}
    assert len(ks) == 8, sorted(ks)   # cls x {dh 64, dh 128, f32}, colsum x {dh 64, dh 128, f32}, the head sum, finish
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['vgpr_count'] <= 128, (n, k)   # four waves per SIMD
    col = {n: k for n, k in ks.items() if 'rollout_colsum_kernel' in n}
    assert sorted(k['group_segment_fixed_size'] for k in col.values()) == [8 * 1024 + 512, 16 * 1024 + 512]   # HI x 8 KiB Q images + lse / w
