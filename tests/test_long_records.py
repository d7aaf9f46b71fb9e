"""CPU: the bf16 engine accepts records of 513 to 2048 tokens (fused attention above 512 tokens), and the kernels that only such records launch
are spill-free and inside their register budgets (code-object metadata, tools/code_objects.py; no GPU)."""
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

import ecg_representation_learning_amd as E
from ecg_representation_learning_amd.engine import VitEngine

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')


def _engine(L, P, d=768, h=12, **kw):
    return VitEngine(C=12, L=L, P=P, d=d, h=h, f=4 * d, Ly=2, K=5, p_hidden=0.1, p_emb=0.1, dtype=kw.pop('dtype', torch.bfloat16), layout=None, **kw)


@pytest.mark.parametrize('L,P,N', [(5000, 4, 1251), (5000, 8, 626), (2560, 2, 1281), (2560, 4, 641), (4094, 2, 2048), (1026, 2, 514)])
def test_bf16_engine_takes_long_records(L, P, N):
    eng = _engine(L, P)
    assert eng.N == N


def test_bf16_engine_rejects_more_than_2048_tokens():
    with pytest.raises(ValueError, match='2048'):
        _engine(4096, 2)                          # 2049 tokens
    assert _engine(4096, 2, dtype=torch.float32).N == 2049   # the f32 path is unchanged


def test_bf16_engine_still_rejects_other_head_dims():
    with pytest.raises(ValueError, match='head dim 64'):
        _engine(5000, 4, d=384, h=12)             # dh = 32


@pytest.fixture(scope='module')
def kernels():
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    return code_objects.kernels(LIB)


def test_long_record_kernels_and_uniform_cls_forward_are_spill_free_and_within_budget(kernels):
    """the instantiations only N > 512 launches: the streamed forward's MODE 4 (<= 128 VGPRs: four waves per SIMD), the persistent backward with
    the 2048-query LSE row (<= 256: two waves per SIMD, and inside 160 KiB of LDS), the dh = 64 CLS-row forward (uniform form; its score array
    holds 2048 keys at every N: <= 128 VGPRs, LDS 8 KiB + 32 x 65 floats + 16 B)"""
    fwd = [n for n in kernels if re.search(r'attn_fwd_stream_kernelILb[01]ELb[01]ELi4EE', n)]
    bwd = [n for n in kernels if 'attn_bwd_pers_kernel' in n and 'Li2048EE' in n]
    cls = [n for n in kernels if 'attnu_cls_fwd_kernelILi1E' in n]
    assert len(fwd) == 4 and len(bwd) == 4 and len(cls) == 2, (fwd, bwd, cls)
    for n in fwd + bwd + cls:
        k = kernels[n]
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (n, k)
    for n in fwd:
        assert kernels[n]['vgpr_count'] <= 128, (n, kernels[n])
    for n in bwd:
        assert kernels[n]['vgpr_count'] + kernels[n]['agpr_count'] <= 256, (n, kernels[n])
        assert kernels[n]['group_segment_fixed_size'] <= 160 * 1024, (n, kernels[n])
    for n in cls:
        assert kernels[n]['vgpr_count'] <= 128 and kernels[n]['group_segment_fixed_size'] <= 16528, (n, kernels[n])
