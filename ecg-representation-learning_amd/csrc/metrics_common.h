// What the evaluation kernels share (metrics.hip: confusion counts and all-pairs AUROC; rank_metrics.hip: the rank route; pr_metrics.hip: average
// precision and F-max): the one definition of the probability a score stands for -- both AUROC routes must compare the same floats, so neither
// restates it -- and the skeleton of a walk over the sorted order, of which rank_walk_kernel and prc_walk_kernel fill in the per-position body.
#pragma once
#include "common.h"
#include "../../include/ecgvit_hip_rank.h"

__device__ __forceinline__ float as_prob(float s, int from_logits) { return from_logits ? 1.0f / (1.0f + expf(-s)) : s; }

// ---- the packed word of a sorted position (include/ecgvit_hip_rank.h) ----------------------------------------------------------------------
#define RANK_INDEX_MASK 0x3FFFFFFFu
#define RANK_LABEL_BIT 0x40000000u
#define RANK_LAST_BIT 0x80000000u
#define WALK_THREADS 256   // four waves; wave (blockIdx.x * 4 + w) of class blockIdx.y carries replicates [wave * GROUP, wave * GROUP + GROUP)
static_assert(ECGVIT_RANK_MAX_ROWS == (1 << 30) && ECGVIT_RANK_GROUP == 4, "index beside two flag bits; a record's multiplicities of one wave are one u32x4");

static __host__ __device__ inline int64_t rank_pad4(int64_t R) { return (R + 3) & ~(int64_t)3; }   // the pitch of the record-major multiplicities

// ---- a walk's wave: every shuffle and ballot below is executed by all 64 lanes ---------------------------------------------------------------
template <typename T> __device__ __forceinline__ T walk_scan(T v, int l) {   // inclusive, along the lanes
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const T u = __shfl_up(v, o, WAVE);
        if (l >= o) v += u;
    }
    return v;
}
template <typename T> __device__ __forceinline__ T walk_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

struct WalkWave {
    const int c, l;             // class; lane
    const int64_t r0, R4;       // first replicate of the wave (wave-uniform: a wave with r0 >= R returns before any cross-lane operation)
    const uint32_t *order;      // the class's row of `packed`
    const uint64_t below;       // the lanes under this one
    __device__ __forceinline__ WalkWave(const uint32_t *packed, int64_t n, int64_t R)
        : c(blockIdx.y), l(threadIdx.x & 63), r0(((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ECGVIT_RANK_GROUP), R4(rank_pad4(R)),
          order(packed + (int64_t)c * n), below((1ull << l) - 1ull) {}
};

// The weights of the position that holds `word`, `at` saying whether the lane holds a position at all: one 16-byte load from the record-major rows
// (a gather by record index fetches a whole cache line whatever it uses of it: replicate-major rows moved sixteen times the bytes).  mult null: ones.
__device__ __forceinline__ void walk_weights(const WalkWave &wv, uint32_t word, bool at, int64_t n, const uint32_t *__restrict__ mult, int64_t R,
                                             uint32_t (&w)[ECGVIT_RANK_GROUP]) {
    const uint32_t i = word & RANK_INDEX_MASK;
    const bool in = at && i < n;
    const u32x4 m = !in ? u32x4{0u, 0u, 0u, 0u} : mult ? *reinterpret_cast<const u32x4 *>(mult + (int64_t)i * wv.R4 + wv.r0) : u32x4{1u, 1u, 1u, 1u};
#pragma unroll
    for (int g = 0; g < ECGVIT_RANK_GROUP; ++g) w[g] = wv.r0 + g < R ? m[g] : 0u;
}

// the lanes that close a tie group in this step: all of them, those under this lane, and the highest lane of either set
struct WalkCloses {
    uint64_t closes, before;
    int prev, top;
};
__device__ __forceinline__ WalkCloses walk_closes(bool any, uint64_t below) {
    const uint64_t closes = __ballot(any), before = closes & below;
    return {closes, before, before ? 63 - __clzll(before) : 0, closes ? 63 - __clzll(closes) : 0};
}

// ---- host side of the two walk launchers -------------------------------------------------------------------------------------------------------
static inline bool rank_shape_ok(int64_t n, int K) { return n >= 1 && n <= ECGVIT_RANK_MAX_ROWS && K >= 1 && K <= ECGVIT_RANK_MAX_CLASSES; }
static inline bool walk_args_ok(const void *packed, const void *first_nan, int64_t n, int K, const void *mult, int64_t R, const void *out) {
    return rank_shape_ok(n, K) && R >= 1 && R <= ECGVIT_RANK_MAX_REPLICATES && packed && first_nan && out && !(reinterpret_cast<uintptr_t>(mult) & 15);
}
static inline dim3 walk_grid(int64_t R, int K) {
    const int64_t per = WALK_THREADS / WAVE * ECGVIT_RANK_GROUP;
    return dim3((unsigned)((R + per - 1) / per), K);
}
