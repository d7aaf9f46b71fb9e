"""CPU: pooled representations -- the `ecgvit_pool_records` entry point is declared, exported and bound without an ABI bump, its argument checks
run on the host, `encode` validates `pool` before anything else and reaches the existing refusals unchanged, and the new kernels carry no spills
(code-object metadata, tools/code_objects.py; no GPU)."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
import abi_header

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip
from ecg_representation_learning_amd.engine import VitEngine

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')
P = 4


def _engine(dtype=torch.bfloat16, N=251, **kw):
    return VitEngine(C=12, L=P * (N - 1), P=P, d=128, h=2, f=256, Ly=2, K=5, p_hidden=0.0, p_emb=0.0, dtype=dtype, layout=None, **kw)


def test_entry_point_declared_exported_and_bound_at_abi_6():
    src = open(abi_header.HEADER).read()
    assert abi_header.held({'ecgvit_pool_records': 13}, hip.SIGNATURES)['ecgvit_pool_records'][0] == 'int'
    assert hasattr(ctypes.CDLL(hip.LIB_PATH), 'ecgvit_pool_records')
    assert hip.ABI_VERSION == 6 and hip.lib().ecgvit_abi_version() == 6
    assert re.search(r'^#define ECGVIT_ABI\s+6\b', src, re.M) or 'abi6' in hip.lib().ecgvit_version().decode()
    assert (hip.POOL_CLS, hip.POOL_MEAN) == (0, 1)


def test_kernel_argument_checks_run_on_the_host():
    """every refusal returns ECGVIT_EINVAL before anything is launched (no pointer is dereferenced)"""
    l = hip.lib()
    x, out, g = 0x10000000, 0x20000000, 0x30000000

    def rc(B=4, N=9, d=64, mode=1, gamma=None, beta=None, dtype=hip.BF16, x=x, out=out):
        return l.ecgvit_pool_records(x, out, None, None, B, N, d, mode, gamma, beta, 1e-5, dtype, None)
    assert rc(d=68) == 1 and rc(d=2056) == 1 and rc(d=0) == 1          # d: a multiple of 8, at most 2048
    assert rc(mode=2) == 1 and rc(mode=-1) == 1
    assert rc(dtype=hip.FP8_E4M3) == 1 and rc(dtype=7) == 1
    assert rc(B=0) == 1 and rc(N=0) == 1
    assert rc(gamma=g) == 1 and rc(beta=g) == 1                         # LayerNorm takes both or neither
    assert rc(x=None) == 1 and rc(out=None) == 1


def test_bad_pool_raises_before_any_device_work():
    x = torch.zeros(2, 12, 1000)
    for dtype in (torch.float32, torch.bfloat16):
        for bad in ('max', 'CLS', None, 0):
            with pytest.raises(ValueError, match='pool'):
                _engine(dtype).encode(x, pool=bad)
            with pytest.raises(ValueError, match='pool'):
                _engine(dtype).pool_saved(pool=bad)
    model = E.EcgVit()
    with pytest.raises(ValueError, match='pool'):
        model.encode(torch.zeros(2, 12, 2560), pool='avg')   # (a host tensor: the pool check comes before the device check)
    with pytest.raises(RuntimeError, match='MI355X'):
        model.encode(torch.zeros(2, 12, 2560))
    with pytest.raises(ValueError, match='pool'):
        E.HipEncoder(model, pool='avg')
    with pytest.raises(ValueError, match='batch_size'):
        E.HipEncoder(model, batch_size=0)


def test_mean_pool_needs_every_row():
    """the compact CLS rows of a pruned last block hold nothing to average"""
    eng = _engine()
    eng.saved = dict(B=2, masked=False, cls_only_last=True, ragged=None, ntok=None, xL=torch.zeros(2, 128))
    with pytest.raises(ValueError, match='mean'):
        eng.pool_saved('mean')
    eng.saved = None
    with pytest.raises(RuntimeError, match='forward'):
        eng.pool_saved('cls')


@pytest.mark.parametrize('pool', ['cls', 'mean'])
def test_existing_refusals_are_reached_unchanged(pool):
    fp8 = VitEngine(C=12, L=P * 250, P=P, d=256, h=4, f=512, Ly=2, K=5, p_hidden=0.0, p_emb=0.0, dtype=torch.bfloat16, layout=None, fp8_linear=True)
    with pytest.raises(ValueError, match='fp8_linear'):
        fp8.encode(torch.zeros(2, 12, 1000), lengths=torch.tensor([1000, 400]), pool=pool)
    with pytest.raises(ValueError, match='fp8_linear'):
        fp8.encode(torch.zeros(2, 12, 600), pool=pool)
    with pytest.raises(ValueError, match='fp8_linear'):
        fp8.encode(torch.zeros(12, 600), lengths=torch.tensor([600]), pool=pool)
    with pytest.raises(ValueError, match='bf16 engine'):
        _engine(torch.float32).encode(torch.zeros(12, 600), lengths=torch.tensor([600]), pool=pool)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(ValueError, match='multiple'):
            _engine(dtype).encode(torch.zeros(2, 12, 600), lengths=torch.tensor([600, 6]), pool=pool)
        with pytest.raises(ValueError, match='exceed'):
            _engine(dtype).encode(torch.zeros(2, 12, 600), lengths=torch.tensor([600, 604]), pool=pool)
    eng = _engine()
    eng.input_transform = E.FusedInputTransform(mean=[0.0] * 12, std=[1.0] * 12, patch_size=P)
    with pytest.raises(ValueError, match='input transform'):
        eng.encode(torch.zeros(2, 12, 998), lengths=torch.tensor([1000, 400]), pool=pool)
    with pytest.raises(ValueError, match='sum to'):
        _engine().encode(torch.zeros(12, 600), lengths=torch.tensor([400, 100]), pool=pool)


def test_public_surface():
    sig = inspect.signature(E.EcgVit.encode).parameters
    assert list(sig) == ['self', 'sample_values', 'lengths', 'pool', 'norm']
    assert (sig['lengths'].default, sig['pool'].default, sig['norm'].default) == (None, 'cls', True)
    sig = inspect.signature(E.HipEncoder.__init__).parameters
    assert (sig['batch_size'].default, sig['pool'].default, sig['norm'].default) == (64, 'cls', True)
    assert list(inspect.signature(E.HipEncoder.encode).parameters) == ['self', 'sample_values', 'lengths']
    assert list(inspect.signature(E.HipProbeStep.step).parameters) == ['self', 'features', 'labels']
    assert issubclass(E.HipProbeStep, E.HipTrainStep)   # get_last_lr / grad_norm / finish: one surface
    st = E.HipProbeStep(E.EcgVit(), dict(n_step=10, warmup_ratio=0.2, learning_rate=1e-2))
    assert st.get_last_lr() == 0.0 and (st.world, st.collectives) == (1, False)
    with pytest.raises(RuntimeError, match='device'):
        st.step(torch.zeros(2, 512), torch.zeros(2, 71))
    with pytest.raises(TypeError):
        st.step_masked(None, None)


def test_pool_kernels_spill_free():
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    ks = {n: k for n, k in code_objects.kernels(LIB).items() if 'pool_records_kernel' in n or 'pool_layernorm_kernel' in n}
    assert len(ks) == 3, sorted(ks)   # f32 and bf16 pooling, the LayerNorm of the pooled vectors
    for n, k in ks.items():
        assert k['vgpr_spill_count'] == 0 and k['sgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
        assert k['vgpr_count'] <= 64 and k['group_segment_fixed_size'] <= 64 * 65 * 4, (n, k)   # 8 waves / SIMD; 64 slots x (64 + 1) f32 columns
