// What the evaluation kernels share (metrics.hip: confusion counts and all-pairs AUROC; rank_metrics.hip: the rank route): the one definition of
// the probability a score stands for.  Both routes must compare the same floats, so neither restates it.
#pragma once
#include "common.h"

__device__ __forceinline__ float as_prob(float s, int from_logits) { return from_logits ? 1.0f / (1.0f + expf(-s)) : s; }
