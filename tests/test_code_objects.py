"""CPU: resources of the shipped library's kernels, read from the code-object metadata (tools/code_objects.py; llvm-readelf, no GPU).
The streaming kernels retire their LDS-DMA pieces with COUNTED `s_waitcnt vmcnt(N)`: a spilled register would add scratch loads / stores to
that count (and to the CU's memory path those kernels are bound by), so every instantiation the train step can launch must be spill-free."""
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tools'))
LIB = os.path.join(ROOT, 'ecg-representation-learning_amd', 'libecgvit_hip.so')


@pytest.fixture(scope='module')
def kernels():
    import code_objects
    if not os.path.exists(code_objects.READELF):
        pytest.skip('llvm-readelf not in this image')
    ks = code_objects.kernels(LIB)
    assert len(ks) > 100, len(ks)
    return ks


def test_streaming_kernels_do_not_spill(kernels):
    counted = ('attn_bwd_pers_kernel', 'attn_fwd_bf16_kernel', 'attn_fwd_stream_kernel', 'gemm_nt_kernel_4w', 'gemm_wgrad_kernel', 'gemm_wgrad8_kernel', 'gemm_nt_kernel')
    seen = 0
    for name, k in kernels.items():
        if not any(c in name for c in counted):
            continue
        if re.search(r'gemm_nt_kernelI\w+?Lin1E', name):     # FLAGS = -1: the run-time-flag fallback bodies (no train-step launch takes them)
            continue
        seen += 1
        assert k['vgpr_spill_count'] == 0 and k['private_segment_fixed_size'] == 0, (name, k)
    assert seen >= 40, seen


# the instantiations of every family: the exact-lane forward at 6 widths x {plain, Q8}, the exact-lane backward at 6 widths x {plain, EXTRA, EXTRA + Q8},
# the generic forward at bf16 MAXV 1, 2, 4 and f32 MAXV 1, 2, 4, 8, the generic backward at the same seven x {plain, EXTRA}, the quantise pass per format
ROW_EMITTERS = {'layernorm_fwd_fit_kernel': 12, 'layernorm_bwd_fit_kernel': 18, 'fp8_quantize_kernel': 2, 'layernorm_fwd_kernel': 7, 'layernorm_bwd_kernel': 14}


@pytest.mark.parametrize('family', list(ROW_EMITTERS))
def test_row_emitters_do_not_spill(kernels, family):
    """every LayerNorm kernel, exact-lane and generic, and the quantise pass, every instantiation: the exact-lane E <= 12 backward sits at 128
    VGPRs under a four-waves-per-SIMD launch bound, where one register more is a spill, not a lower occupancy.  (That backward used to spill at
    E = 12 with the third sum and at E = 32, up to 56 VGPRs, on loop-invariant per-lane pointers: profiles/r31_q8_encoder.txt (b).)"""
    mine = {name: k for name, k in kernels.items() if family in name}
    assert len(mine) == ROW_EMITTERS[family], sorted(mine)
    spilling = {name: (k['vgpr_spill_count'], k['private_segment_fixed_size']) for name, k in mine.items()
                if k['vgpr_spill_count'] or k['private_segment_fixed_size']}
    assert not spilling, spilling


def test_persistent_kernels_keep_their_occupancy(kernels):
    """register counts that decide how many waves share a SIMD: the eight-wave bodies <= 256 (two waves), the four-wave bodies <= 512 (one),
    the attention forward <= 128 (four)"""
    for name, k in kernels.items():
        if 'attn_fwd_bf16_kernel' in name or 'attn_fwd_stream_kernel' in name:   # (the streamed forward: sixteen waves per workgroup = four per SIMD)
            assert k['vgpr_count'] <= 128, (name, k)
        elif 'attn_bwd_pers_kernel' in name or re.search(r'gemm_nt_kernelI', name) or re.search(r'gemm_wgrad8?_kernelI', name):
            assert k['vgpr_count'] <= 256, (name, k)
        elif 'kernel_4w' in name:
            assert k['vgpr_count'] <= 512, (name, k)
