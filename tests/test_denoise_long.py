"""CPU: the Holter-length entry points of csrc/denoise.hip (`ecgvit_*_long`, `ecgvit_*_tiled`) -- symbols and arity, every refusal of their
launchers (no GPU is touched: a refused call launches nothing), the workspace formula at the INCART length, the kernels the two caps share, the
resources of the new kernels, and the host contract of `tiled=` / `tile=` in `denoise`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import abi_header
import ecg_representation_learning_amd as E
from ecg_representation_learning_amd import hip, denoise
from ecg_representation_learning_amd.records import DeviceTables

HEADER = abi_header.HEADER
CAP = 1 << 25
INCART = 462600
ARITY = {'ecgvit_denoise_workspace_long': 3, 'ecgvit_filtfilt_long': 15, 'ecgvit_nlm_sigma_long': 10, 'ecgvit_nlm_denoise_tiled': 14,
         'ecgvit_rloess_tiled': 17}
PRESENT = {'ecgvit_denoise_workspace_long': 'ecgvit_denoise_workspace', 'ecgvit_filtfilt_long': 'ecgvit_filtfilt', 'ecgvit_nlm_sigma_long': 'ecgvit_nlm_sigma'}


def test_symbols_exist_with_the_declared_arity():
    lib = hip.lib()
    abi_header.held(ARITY, hip.SIGNATURES)                  # declared, with this many arguments, bound with the declaration's types
    for name in ARITY:
        assert hasattr(lib, name)
    for name, present in PRESENT.items():                   # the _long forms take the arguments of the present entry points
        assert hip.SIGNATURES[name] == hip.SIGNATURES[present], name
    assert hip.SIGNATURES['ecgvit_nlm_denoise_tiled'][1][:12] == hip.SIGNATURES['ecgvit_nlm_denoise'][1][:12]
    assert hip.SIGNATURES['ecgvit_rloess_tiled'][1][:15] == hip.SIGNATURES['ecgvit_rloess'][1][:15]
    assert lib.ecgvit_abi_version() == 6
    assert hip.DENOISE_MAX_LEN == denoise.MAX_LEN == 32768 and hip.DENOISE_MAX_LEN_TILED == denoise.MAX_LEN_TILED == CAP


def test_the_header_states_the_contracts():
    src = ' '.join(open(HEADER).read().split())
    assert 'bit-identical to ecgvit_nlm_denoise for every * n <= ECGVIT_DENOISE_MAX_LEN and every tile_runs' in src
    assert 'bit-identical to ecgvit_rloess for every n <= ECGVIT_DENOISE_MAX_LEN and every tile_samples' in src
    assert '#define ECGVIT_DENOISE_MAX_LEN 32768 ' in src
    assert 'out == x is REFUSED' in src


def test_workspace_formula():
    l = hip.lib()
    assert l.ecgvit_denoise_workspace_long(75, 12, INCART) == 75 * 12 * (INCART + 64) * 8
    assert l.ecgvit_denoise_workspace_long(4, 12, 5000) == l.ecgvit_denoise_workspace(4, 12, 5000) == 4 * 12 * (5000 + 64) * 8
    assert l.ecgvit_denoise_workspace_long(1, 12, CAP) == 12 * (CAP + 64) * 8
    assert l.ecgvit_denoise_workspace_long(1, 12, CAP + 1) == 0 and l.ecgvit_denoise_workspace_long(0, 12, 64) == 0
    assert l.ecgvit_denoise_workspace_long(4, 0, 64) == 0 and l.ecgvit_denoise_workspace_long(4, 12, 0) == 0
    assert l.ecgvit_denoise_workspace(4, 12, 32769) == 0                  # the present cap stays


# ---- refusals ---------------------------------------------------------------------------------------------
P = 0x10000000      # never dereferenced: a refused call launches nothing
Q = 0x20000000
B4 = (ctypes.c_double * 4)(0.1, 0.3, 0.3, 0.1)
A4 = (ctypes.c_double * 4)(1.0, -0.5, 0.2, -0.1)
Z3 = (ctypes.c_double * 3)(0.9, -0.2, 0.1)
IDS = dict(ids=lambda d: ','.join(f'{k}={v if not isinstance(v, ctypes.Array) else list(v)}' for k, v in d.items()))


def _filt(**kw):
    a = dict(x=P, out=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, min_len=64, max_len=64, b=B4, a=A4, zi=Z3, ntaps=4, workspace=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_filtfilt_long(*a.values())


def _sigma(**kw):
    a = dict(x=P, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, max_len=64, sigma=P, workspace=P, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_nlm_sigma_long(*a.values())


def _nlm(**kw):
    a = dict(x=P, out=Q, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, max_len=64, sigma=P, scale=1.5, patch_wd=10, sch_wd=0, tile_runs=0, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_nlm_denoise_tiled(*a.values())


def _rloess(**kw):
    a = dict(x=P, out=Q, src_off=P, lead_stride=64, raw_len=P, R=4, C=12, min_len=64, max_len=64, npoints=31, frac=0.0, degree=2, robust_iters=10,
             subtract=0, iters=None, tile_samples=0, stream=None)
    a.update(kw)
    return hip.lib().ecgvit_rloess_tiled(*a.values())


BAD_STORE = [dict(x=None), dict(x=P + 2), dict(src_off=None), dict(src_off=P + 4), dict(raw_len=None), dict(raw_len=P + 2), dict(R=0), dict(R=-1), dict(C=0),
             dict(C=65536), dict(max_len=0), dict(max_len=-5), dict(max_len=CAP + 1)]


@pytest.mark.parametrize('bad', BAD_STORE + [dict(out=None), dict(out=P + 2), dict(workspace=None), dict(workspace=P + 4), dict(b=None), dict(a=None), dict(zi=None),
                                             dict(ntaps=0), dict(ntaps=10), dict(min_len=12, ntaps=4), dict(min_len=0), dict(min_len=65),
                                             dict(a=(ctypes.c_double * 4)(2.0, 0, 0, 0)), dict(b=(ctypes.c_double * 4)(float('nan'), 0, 0, 0))], **IDS)
def test_filtfilt_long_refusals(bad):
    assert _filt(**bad) == 1


@pytest.mark.parametrize('bad', BAD_STORE + [dict(sigma=None), dict(sigma=P + 4), dict(workspace=None), dict(workspace=P + 4)], **IDS)
def test_sigma_long_refusals(bad):
    assert _sigma(**bad) == 1


@pytest.mark.parametrize('bad', BAD_STORE + [dict(out=None), dict(out=Q + 2), dict(out=P), dict(sigma=None), dict(sigma=P + 4), dict(patch_wd=0), dict(patch_wd=-1),
                                             dict(patch_wd=CAP + 1), dict(sch_wd=-1), dict(scale=0.0), dict(scale=float('nan')), dict(scale=float('inf')),
                                             dict(tile_runs=-1), dict(max_len=CAP, tile_runs=1), dict(max_len=15 * 65536 + 21, tile_runs=1)], **IDS)
def test_nlm_tiled_refusals(bad):
    assert _nlm(**bad) == 1             # out=P: out == x


@pytest.mark.parametrize('bad', BAD_STORE + [dict(out=None), dict(out=Q + 2), dict(out=P), dict(lead_stride=0), dict(degree=0), dict(degree=3), dict(robust_iters=-1),
                                             dict(robust_iters=11), dict(subtract=2), dict(frac=-0.1), dict(frac=1.5), dict(min_len=3), dict(min_len=65),
                                             dict(npoints=3), dict(npoints=1025, max_len=2000), dict(frac=0.9, max_len=2000, min_len=2000),
                                             dict(tile_samples=-1), dict(tile_samples=4097),
                                             dict(tile_samples=4096 - 2 * 31 + 1),                                   # tile + two windows of 31 over the LDS array
                                             dict(tile_samples=2049, npoints=1024, max_len=5000, min_len=5000),      # the same at the widest window
                                             dict(tile_samples=3969, npoints=1024),                                  # the window is the record's 64 samples here
                                             dict(tile_samples=64, max_len=64 * 65535 + 1)], **IDS)
def test_rloess_tiled_refusals(bad):
    assert _rloess(**bad) == 1


# ---- the built library --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kernels():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import code_objects
    return code_objects.kernels(hip.LIB_PATH)


def test_the_two_caps_share_one_kernel(kernels):
    assert sum('filtfilt_kernel' in k for k in kernels) == 1 and sum('nlm_sigma_kernel' in k for k in kernels) == 1


def test_new_kernels_have_no_spills_and_no_scratch(kernels):
    new = {k: v for k, v in kernels.items() if 'nlm_tiled_kernel' in k or 'rloess_tiled_kernel' in k}
    assert len(new) == 6, sorted(new)                      # one non-local means, five slot counts of the LOESS
    for k, v in new.items():
        assert v['vgpr_spill_count'] == 0 and v['private_segment_fixed_size'] == 0, (k, v)         # what tools/code_objects.py lists: no spill, no scratch
        assert v['group_segment_fixed_size'] == (16384 if 'rloess' in k else 2 * (256 + 14 + 20) * 4), (k, v)


# ---- host contract ----------------------------------------------------------------------------------------
def test_host_refusals():
    x = torch.zeros(2, 12, 64)
    assert denoise.MAX_LEN == 32768 and denoise.MAX_LEN_TILED == CAP
    stages = (E.lowpass, E.estimate_noise_std, E.nlm, E.rloess, E.EcgDenoiser())
    for fn in stages:
        with pytest.raises(ValueError, match='32768'):                   # tiled=False keeps the present cap
            fn(np.zeros((1, 12, 32769), np.float32))
        with pytest.raises(ValueError, match='tiled=True'):              # a tile without tiled
            fn(x, tile=30)
        for bad in (0, -15, 2.5, True, '30'):
            with pytest.raises(ValueError, match='tile'):
                fn(x, tiled=True, tile=bad)
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (1, 12, CAP + 1), (0, 0, 0))       # one float of memory
    for fn in stages:
        with pytest.raises(ValueError, match=str(CAP)):                  # over the tiled cap: names that number
            fn(big, tiled=True)
    for fn in (E.nlm, E.EcgDenoiser()):
        with pytest.raises(ValueError, match='multiple of 15'):
            fn(x, tiled=True, tile=64)
    with pytest.raises(ValueError, match='fit'):                          # the tile and two windows of 64 samples: at most 3968
        E.rloess(x, 500, tiled=True, tile=3969)
    with pytest.raises(ValueError, match='fit'):
        E.rloess(np.zeros((1, 12, 3000), np.float32), 1024, tiled=True, tile=2049)
    with pytest.raises(ValueError, match='fit'):
        E.EcgDenoiser()(np.zeros((1, 12, 3000), np.float32), baseline='rloess', tiled=True, tile=3105)
    with pytest.raises(ValueError, match='tiles'):
        E.rloess(np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (1, 12, 64 * 65535 + 1), (0, 0, 0)), 31, tiled=True, tile=64)
    if not torch.cuda.is_available():
        for fn in stages:
            with pytest.raises(RuntimeError, match='no CPU fallback'):   # every other check passed: only the device is missing
                fn(np.zeros((1, 12, 40000), np.float32), tiled=True)


def test_launch_groups_at_the_incart_length():
    tab = DeviceTables.__new__(DeviceTables)
    tab.R, tab.max_len = 75, INCART
    ws = [cnt * hip.lib().ecgvit_denoise_workspace_long(1, 12, INCART) for _, cnt in denoise.launches(tab, denoise._ENTRY[True])]
    assert max(ws) <= denoise._WS_BYTES and sum(cnt for _, cnt in denoise.launches(tab, denoise._ENTRY[True])) == 75
    groups = denoise.groups(tab)
    assert max(cnt for _, cnt in groups) * 12 * INCART * 4 <= denoise._WS_BYTES and sum(cnt for _, cnt in groups) == 75
    assert [lo for lo, _ in groups] == list(np.cumsum([0] + [cnt for _, cnt in groups])[:-1])
