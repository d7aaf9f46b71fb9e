"""
ctypes table of `include/ecgvit_hip_pr.h`: average precision and class-wise F-max on the sorted order of the rank route, exported by the one
library (`hip.LIB_PATH`) and typed on it at first use (`hip.bind`).  A table of its own, as `rank_abi.py` is: the header is one of its own.  Every
call goes through `run`, the checked-call mechanism of `hip.run` over this table.  tests/test_pr_metrics.py holds the table to the header, type by
type, and the constants below to its defines.
"""
from ctypes import c_int, c_int64, c_void_p

from . import hip

# constants of the header (`ECGVIT_PR_X` there is `X` here)
SLOTS = 6                   # int64 per (replicate, class): ap_q, wp, wn, f_tp, f_fp, f_pos
MAX_WEIGHT = 1073741824     # the weights of one replicate sum to less than this (1 << 30)

_P, _I, _L = c_void_p, c_int, c_int64
SIGNATURES = {
    'ecgvit_pr_walk': (c_int, [_P, _P, _L, _I, _P, _L, _P, _P]),
}

run = hip._Run(SIGNATURES)


def lib():
    return hip.bind(SIGNATURES)
