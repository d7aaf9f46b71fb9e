"""
ctypes table of `include/ecgvit_hip_knn.h`: the k-NN search, merge, normalise and vote entry points, exported by the one library
(`hip.LIB_PATH`) beside those of `include/ecgvit_hip.h` and typed on it at first use (`hip.bind`).  A table of its own, not rows of
`hip.SIGNATURES`: the header is one of its own.  Every call goes through `run`, the checked-call mechanism of `hip.run` over this table; the
size queries through `lib()`.  tests/test_knn.py holds the table to the header, type by type, and the limits below to its defines.
"""
from ctypes import c_int, c_int64, c_double, c_void_p

from . import hip

# limits and constants of the header (`ECGVIT_KNN_X` there is `X` here)
MAX_K = 256              # neighbours per query
MAX_SPLITS = 1024        # row ranges of the bank
TILE = 128               # queries and bank rows per score tile
MAX_ROWS = 2147483520    # N of a search (2^31 - 128)
MAX_PITCH = 16777216     # ldq, ldb of a search
MAX_MERGE = 1048576      # P * k_p of a merge
MAX_CLASSES = 65536      # label columns of a vote
VOTE_UNIFORM, VOTE_SOFTMAX = 0, 1

_P, _I, _L, _D = c_void_p, c_int, c_int64, c_double
SIGNATURES = {
    'ecgvit_knn_splits': (c_int, [_L, _L, _I]),
    'ecgvit_knn_workspace': (c_int64, [_L, _L, _I, _I, _I]),
    'ecgvit_knn_search': (c_int, [_P, _L, _P, _L, _L, _L, _I, _I, _L, _L, _I, _P, _P, _P, _P]),
    'ecgvit_knn_merge': (c_int, [_P, _P, _I, _L, _L, _L, _I, _I, _L, _P, _P, _P]),
    'ecgvit_knn_normalize': (c_int, [_P, _L, _P, _L, _L, _I, _P]),
    'ecgvit_knn_vote': (c_int, [_P, _P, _L, _I, _P, _L, _L, _I, _I, _D, _P, _P]),
}

run = hip._Run(SIGNATURES, queries=('ecgvit_knn_splits',))


def lib():
    return hip.bind(SIGNATURES)
