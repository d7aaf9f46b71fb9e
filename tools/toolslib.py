"""ctypes binding of the TOOLS build of the library (tools/ecgvit_hip_tools.h; `make -C ecg-representation-learning_amd/csrc tools`):
the product C-ABI plus the test / diagnostic entry points.  Used by tests/hiputil.py and tools/*.py -- never by the product package."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TOOLS_LIB_PATH = os.path.join(ROOT, 'ecg-representation-learning_amd', 'csrc', 'build', 'libecgvit_hip_tools.so')
_P, _I, _F, _U = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint64
SIGNATURES = {   # name -> (restype, argtypes); mirrors tools/ecgvit_hip_tools.h (tests/test_abi.py); tools/gemm_ab.py binds ecgvit_tools_gemm itself
    'ecgvit_probe_mfma_layout': (_I, [_P, _P]),
    'ecgvit_attention_bwd_oneitem': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _F, _U, _I, _P]),
    'ecgvit_tools_attn_fwd_variant': (_I, [_I]),
    'ecgvit_tools_resample_pass': (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    'ecgvit_tools_resample_chirp': (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _P, _P]),
}
_tools = None


def tools_lib():
    global _tools
    if _tools is None:
        from ecg_representation_learning_amd import hip
        if not os.path.exists(TOOLS_LIB_PATH):
            raise hip.HipLibraryMissing(f'{TOOLS_LIB_PATH} not found: build it with `make -C ecg-representation-learning_amd/csrc tools` '
                                        f'(__graft_entry__.build() does)')
        l = ctypes.CDLL(TOOLS_LIB_PATH)
        for name, (res, args) in {**hip.SIGNATURES, **SIGNATURES}.items():      # the product entry points of the same build, then the tools'
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _tools = l
    return _tools
