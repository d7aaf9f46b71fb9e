"""CPU: the C-ABI library loads and exports every symbol include/ecgvit_hip.h declares; the ctypes tables are the headers, type by type; the
binding's constants are the header's defines."""
import ctypes
import os
import re
import sys

import pytest

from conftest import ROOT
import abi_header
import ecg_representation_learning_amd as E


def declared_symbols():
    return sorted(abi_header.declarations())


def test_signatures_are_the_headers_argument_by_argument():
    """hip.SIGNATURES against every declaration of include/ecgvit_hip.h: the names in both directions, the return type and every argument
    type (an `_I` where the header says int64_t, an `_F` where it says double puts the wrong thing in a register)"""
    decls = abi_header.declarations()
    assert len(decls) == 108 == len(E.hip.SIGNATURES)
    assert abi_header.mismatches(E.hip.SIGNATURES, decls, E.hip.GemmDesc) == []
    assert E.hip.SIGNATURES['ecgvit_gemm'][1][0] is ctypes.POINTER(E.hip.GemmDesc) and E.hip.SIGNATURES['ecgvit_version'][0] is ctypes.c_char_p


def test_mismatches_reports_each_kind_of_difference():
    """the comparison itself: one int64_t bound as int, one double bound as float and one argument dropped give exactly three entries (a parser
    that matches nothing, or a comparison that accepts anything, would pass the test above)"""
    hip, decls = E.hip, abi_header.declarations()
    table = {n: (r, list(a)) for n, (r, a) in hip.SIGNATURES.items()}
    i = table['ecgvit_fp8_amax'][1].index(hip._L)
    table['ecgvit_fp8_amax'][1][i] = hip._I
    j = table['ecgvit_nlm_denoise'][1].index(hip._D)
    table['ecgvit_nlm_denoise'][1][j] = hip._F
    del table['ecgvit_fit_select'][1][-2]
    assert sorted(abi_header.mismatches(table, decls, hip.GemmDesc)) == [
        'ecgvit_fit_select: 6 parameters, the table has 5',
        f'ecgvit_fp8_amax: parameter {i} is int64_t, the table says c_int',
        f'ecgvit_nlm_denoise: parameter {j} is double, the table says c_float']
    del table['ecgvit_softmax_rows']                         # and both directions of the names, and the return type
    table['ecgvit_nonesuch'] = (hip._I, [])
    table['ecgvit_sumsq_workspace'] = (hip._I, [hip._L])
    assert sorted(abi_header.mismatches(table, decls, hip.GemmDesc))[3:] == [
        'ecgvit_nonesuch: in the table, not declared', 'ecgvit_softmax_rows: declared, not in the table',
        'ecgvit_sumsq_workspace: returns int64_t, the table says c_int']


def test_tools_signatures_are_the_tools_header():
    """the tools binding's own table against tools/ecgvit_hip_tools.h (ecgvit_tools_gemm is bound by tools/gemm_ab.py alone, on the library it loads)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import toolslib
    decls = abi_header.declarations(abi_header.TOOLS_HEADER)
    assert set(decls) - set(toolslib.SIGNATURES) == {'ecgvit_tools_gemm'} and len(toolslib.SIGNATURES) == 5
    assert abi_header.mismatches(toolslib.SIGNATURES, {n: decls[n] for n in toolslib.SIGNATURES}, E.hip.GemmDesc) == []
    assert abi_header.accepts(ctypes.POINTER(E.hip.GemmDesc), decls['ecgvit_tools_gemm'][1][0], E.hip.GemmDesc)


def test_library_exports_every_declared_symbol():
    if not os.path.exists(E.hip.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(E.hip.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/ecgvit_hip.h but not exported'
    assert set(syms) == set(E.hip.SIGNATURES), set(syms) ^ set(E.hip.SIGNATURES)


def test_tools_header_symbols_live_in_the_tools_library_only():
    """tools/ecgvit_hip_tools.h (probes, the one-item attention backward, A/B switches) lives in build/libecgvit_hip_tools.so only: the
    product library exports none of it, the product binding names none of it"""
    tsyms = sorted(abi_header.declarations(abi_header.TOOLS_HEADER))
    assert 'ecgvit_probe_mfma_layout' in tsyms and 'ecgvit_attention_bwd_oneitem' in tsyms and 'ecgvit_tools_attn_fwd_variant' in tsyms
    tools_path = os.path.join(os.path.dirname(E.hip.LIB_PATH), 'csrc', 'build', 'libecgvit_hip_tools.so')
    if not os.path.exists(tools_path):
        import __graft_entry__
        __graft_entry__.build()
    tl, pl = ctypes.CDLL(tools_path), ctypes.CDLL(E.hip.LIB_PATH)
    for s_ in tsyms:
        assert hasattr(tl, s_), f'{s_} declared in tools/ecgvit_hip_tools.h but not exported by the tools library'
        assert not hasattr(pl, s_), f'{s_} is a tools entry point but the PRODUCT library exports it'
        assert s_ not in E.hip.SIGNATURES
    for s_ in declared_symbols():          # the tools library is the product ABI plus the above
        assert hasattr(tl, s_)


def test_version_and_abi():
    l = E.hip.lib()
    assert l.ecgvit_abi_version() == 6
    assert b'gfx950' in l.ecgvit_version()
    assert l.ecgvit_version().decode().endswith(f'abi{l.ecgvit_abi_version()}')   # the two identity calls agree


def test_gemm_desc_matches_header_field_order():
    """names, order AND types of the descriptor's fields"""
    fields = abi_header.desc_fields()
    assert len(fields) == 40 and [name for _, name in fields] == [f[0] for f in E.hip.GemmDesc._fields_]
    assert abi_header.field_mismatches(E.hip.GemmDesc._fields_, fields) == []
    wrong = [(n, ctypes.c_int64 if n == 'K' else ctypes.c_int32 if n == 'ldq8' else t) for n, t in E.hip.GemmDesc._fields_]
    assert abi_header.field_mismatches(wrong, fields) == ['field 6: int32_t K, _fields_ has c_long K', 'field 34: int64_t ldq8, _fields_ has c_int ldq8']


def test_gemm_kernel_route_query_is_host_only():
    """ecgvit_gemm_kernel answers which kernel family ecgvit_gemm would launch -- pure host logic (nothing is launched, no pointer is
    dereferenced), so it runs without a GPU: the dispatch bench.py's probe relies on, pinned per launch type of the train step"""
    hip = E.hip
    l = hip.lib()

    def route(layout, dtype, out_dtype, M, N, K, lda, ldb, ldc, epilogue=0, aux=False, res=False, ws=False):
        d = hip.GemmDesc()
        d.layout, d.dtype, d.out_dtype, d.epilogue = layout, dtype, out_dtype, epilogue
        d.M, d.N, d.K, d.batch1, d.batch2 = M, N, K, 1, 1
        d.A, d.B, d.C = 0x10000000, 0x20000000, 0x30000000           # never dereferenced: alignment is all that is looked at
        d.lda, d.ldb, d.ldc = lda, ldb, ldc
        d.bias = 0x40000000
        d.alpha = 1.0
        if aux:
            d.aux, d.ldaux = 0x50000000, N
        if res:
            d.residual, d.ldr = 0x60000000, N
        if ws:
            d.workspace, d.workspace_bytes, d.colsum_out = 0x70000000, 1 << 30, 0x78000000
        return l.ecgvit_gemm_kernel(ctypes.byref(d))
    M, dm, f = 512 * 251, 768, 3072
    UP = hip.EPI_BIAS | hip.EPI_GELU | hip.EPI_GELU_GRAD_AUX | hip.EPI_DROPOUT
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, M, 3 * dm, dm, dm, dm, 3 * dm) == hip.KERNEL_GEMM_NT                       # QKV forward
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, M, f, dm, dm, dm, f, epilogue=UP, aux=True) == hip.KERNEL_GEMM_NT            # FFN-up forward
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, M, f, dm, dm, dm, f, epilogue=hip.EPI_MUL_AUX | hip.EPI_COLSUM, aux=True, ws=True) == hip.KERNEL_GEMM_NT
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, 2000, dm, dm, dm, dm, dm) == hip.KERNEL_GEMM_BF16                             # short batch: 128^2 kernel
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, M // 251 * 250, dm, 240, 240, 240, dm, epilogue=hip.EPI_BIAS) == hip.KERNEL_GEMM_BF16   # patch embed (K = 240)
    assert route(hip.GEMM_TN, hip.BF16, hip.F32, 3 * dm, dm, M, 3 * dm, dm, dm, ws=True) == hip.KERNEL_GEMM_WGRAD                 # QKV weight gradient
    assert route(hip.GEMM_TN, hip.BF8_E5M2, hip.F32, 3072, 1024, 256 * 501, 3072, 1024, 1024, ws=True) == hip.KERNEL_GEMM_WGRAD   # 8-bit weight gradient
    assert route(hip.GEMM_NT, hip.FP8_E4M3, hip.BF16, 256 * 501, 4096, 1024, 1024, 1024, 4096) == hip.KERNEL_GEMM_NT              # 8-bit forward
    assert route(hip.GEMM_NT, hip.FP8_E4M3, hip.BF16, 1000, 4096, 1024, 1024, 1024, 4096) == hip.KERNEL_NONE                      # 8-bit: large shapes only
    assert route(hip.GEMM_NN, hip.F32, hip.F32, 100, 64, 32, 32, 64, 64) == hip.KERNEL_GEMM_F32
    assert route(hip.GEMM_NT, hip.BF16, hip.BF16, M, dm + 4, dm, dm, dm, dm + 4) == hip.KERNEL_NONE                              # N % 8 != 0: rejected
    assert l.ecgvit_gemm_kernel(None) == hip.KERNEL_NONE


def test_gemm_route_and_workspace_table():
    """ecgvit_gemm_kernel and ecgvit_gemm_workspace over the descriptor sweep of tests/gemm_cases.py (every layout x operand / output type,
    the engine's epilogue flag sets plus invalid ones, both sides of every routing threshold) against tests/golden/gemm_routes.json.
    The fixture was recorded from the library before the GEMM planner; the calls that library routed and then failed or would have faulted
    on (COLSUM off the fused bodies with N or ldc not a multiple of 8, or with no stored C; 8-bit COLSUM products with a null or misaligned
    operand, or ldc / ldaux not a multiple of 8) were then set to ECGVIT_KERNEL_NONE.  Re-record: `python tests/gemm_cases.py [library]`."""
    import gemm_cases
    digest, want = gemm_cases.read_fixture()
    cases = gemm_cases.cases()
    assert len(cases) > 3000 and gemm_cases.labels_digest([label for label, _ in cases]) == digest
    l = E.hip.lib()
    bad = [(label, w, g) for (label, c), w in zip(cases, want) if (g := list(gemm_cases.query(l, c))) != w]
    assert not bad, (len(bad), bad[:20])
    assert l.ecgvit_gemm_workspace(None) == 0


def test_binding_constants_are_the_headers():
    """two-sided: every numeric #define of include/ecgvit_hip.h (dtype / layout / epilogue / kernel-family / mode codes, limits and tile constants)
    is an attribute of the binding with that value, `ECGVIT_X` <-> `hip.X` (the three status codes are held through `hip._ERR`), and every
    all-capitals integer of the binding is such a define (ABI_VERSION is what ecgvit_abi_version() returns: test_version_and_abi)"""
    hip = E.hip
    text = open(os.path.join(ROOT, 'include', 'ecgvit_hip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define ECGVIT_([A-Z0-9_]+)\s+(-?\d+)\b', text, re.M)}
    assert len(defs) >= 53, defs
    status = {'OK', 'EINVAL', 'ELAUNCH'}
    checked = 0
    for name, val in defs.items():
        if name not in status:
            assert type(getattr(hip, name, None)) is int and getattr(hip, name) == val, (name, val, getattr(hip, name, None))
            checked += 1
    mirrored = {n for n, v in vars(hip).items() if n.isupper() and type(v) is int} - {'ABI_VERSION'}
    assert mirrored == set(defs) - status, mirrored ^ (set(defs) - status)
    for need in ('F32', 'BF16', 'FP8_E4M3', 'BF8_E5M2', 'GEMM_NT', 'GEMM_NN', 'GEMM_TN', 'EPI_BIAS', 'EPI_GELU', 'EPI_GELU_BWD', 'EPI_RESIDUAL', 'EPI_ACCUM',
                 'EPI_DROPOUT', 'EPI_COLSUM', 'EPI_GELU_GRAD_AUX', 'EPI_MUL_AUX', 'EPI_QUANT_OUT', 'EPI_NO_OUT', 'KERNEL_NONE', 'KERNEL_GEMM_F32',
                 'KERNEL_GEMM_BF16', 'KERNEL_GEMM_NT', 'KERNEL_GEMM_WGRAD', 'EPI_AUX8', 'ACC_INIT', 'ACC_ADD', 'ACC_FOLD', 'POOL_CLS', 'POOL_MEAN', 'ATTN_MAX_N', 'ROW_MAX_D',
                 'FIT_TARGETS', 'FIT_BINS', 'DENOISE_MAX_LEN', 'DENOISE_MAX_LEN_TILED', 'DENOISE_MAX_TAPS', 'DENOISE_MAX_POINTS',
                 'DENOISE_MAX_ROBUST_ITERS', 'DENOISE_NLM_RUN', 'DENOISE_NLM_MAX_THREADS', 'DENOISE_LOESS_LDS', 'DENOISE_MAX_TILES', 'RESAMPLE_MAX_LEN',
                 'RESAMPLE_MAX_CHIRP', 'RESAMPLE_MAX_GENERIC', 'RESAMPLE_MAX_GRID_Y', 'TOK_MAX_CLUSTERS', 'TOK_MAX_LOCAL_TRIALS', 'TOK_SEED_SPAN',
                 'TOK_DBSCAN_TILE'):
        assert need in defs and hasattr(hip, need), need
    assert checked >= 50
    assert hip.DENOISE_MAX_LEN_TILED == hip.RESAMPLE_MAX_LEN == 1 << 25 and hip.RESAMPLE_MAX_CHIRP == 1 << 24
    assert E.hip.lib().ecgvit_tok_dbscan_tile() == hip.TOK_DBSCAN_TILE
    assert {1: 'EINVAL', 2: 'ELAUNCH'} == {defs['EINVAL']: 'EINVAL', defs['ELAUNCH']: 'ELAUNCH'} and set(hip._ERR) == {1, 2}
