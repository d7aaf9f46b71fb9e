"""
ctypes table of `include/ecgvit_hip_rank.h`: the rank route to AUROC (sort, multiplicities, weighted rank sum), exported by the one library
(`hip.LIB_PATH`) beside the entry points of `include/ecgvit_hip.h` and typed on it at first use (`hip.bind`).  A table of its own, not rows of
`hip.SIGNATURES`: the header is one of its own.  Every call goes through `run`, the checked-call mechanism of `hip.run` over this table; the
size query through `lib()`.  tests/test_rank_metrics.py holds the table to the header, type by type, and the limits below to its defines.
"""
from ctypes import c_int, c_int64, c_uint64, c_void_p

from . import hip

# limits and constants of the header (`ECGVIT_RANK_X` there is `X` here)
TILE = 2048                 # rows per workgroup of a sort pass
SCAN_BATCH = 8              # tiles per step of the scan over a digit's tiles
GROUP = 4                   # replicates a wave of the walk carries beside each other
WALK_ROWS = 256             # sorted positions per step of a wave of the walk
MAX_ROWS = 1073741824       # n (1 << 30)
MAX_CLASSES = 65535         # K
MAX_REPLICATES = 1048576    # R of one call

_P, _I, _L, _U = c_void_p, c_int, c_int64, c_uint64
SIGNATURES = {
    'ecgvit_rank_workspace': (c_int64, [_L, _I, _L]),
    'ecgvit_rank_sort': (c_int, [_P, _L, _P, _L, _L, _I, _I, _P, _P, _P, _P]),
    'ecgvit_rank_multiplicities': (c_int, [_P, _L, _L, _L, _P, _P]),
    'ecgvit_rank_multiplicities_seeded': (c_int, [_U, _L, _L, _L, _P, _P]),
    'ecgvit_rank_walk': (c_int, [_P, _P, _L, _I, _P, _L, _P, _P, _P]),
}

run = hip._Run(SIGNATURES)


def lib():
    return hip.bind(SIGNATURES)
