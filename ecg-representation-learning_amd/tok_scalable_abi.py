"""
ctypes table of `include/ecgvit_hip_tok_scalable.h`: the scalable k-means++ seeding's entry points, exported by the one library (`hip.LIB_PATH`)
beside those of `include/ecgvit_hip.h` and typed on it at first use (`hip.bind`).  A table of its own, not rows of `hip.SIGNATURES`: the
header is one of its own.  Every call goes through `run`, the checked-call mechanism of `hip.run` over this table; the size query through `lib()`.
tests/test_tokenizer_scalable.py holds the table to the header, type by type, and the limits below to its defines.
"""
from ctypes import c_int, c_int64, c_uint64, c_void_p, POINTER

from . import hip

# limits and tile constants of the header (`ECGVIT_TOK_SCALABLE_X` there is `X` here)
MAX_ROUNDS = 16      # n_rounds
FOLD_ROWS = 256      # table rows per LDS chunk of the fold's row stream
SELECT_SPAN = 256    # consecutive positions of one lead per workgroup of the selection
INFO_HEAD = 4        # words of `info` before the per-round blocks

_P, _I, _L, _U = c_void_p, c_int, c_int64, c_uint64
SIGNATURES = {
    'ecgvit_tok_scalable_workspace': (c_int64, [_I, _L, _I, _I, _I, _I, _L]),
    'ecgvit_tok_scalable_seed': (c_int, [_P, _P, _L, _P, _P, _P, _L, _I, _I, _L, _I, _I, _I, _I, _I, _L, _L, _L, POINTER(c_uint64), _U, _P, _P, _P, _P,
                                         _P, _P, _P, _I, _P]),
}

run = hip._Run(SIGNATURES)


def lib():
    return hip.bind(SIGNATURES)


def info_words(n_rounds):
    """uint64 words of `info`: the head, selected[R], truncated[R], pots[R + 1]"""
    return INFO_HEAD + 3 * n_rounds + 1
