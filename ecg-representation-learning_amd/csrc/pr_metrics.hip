// Average precision and class-wise F-max on the sorted order of rank_metrics.hip: a second walk over the packed rows, from the
// highest score down.  Contract, integer forms and limits: include/ecgvit_hip_pr.h.  Everything the device produces is an exact integer; no
// atomics (a wave owns its outputs: plain stores), no floating point, no kernel that waits for another workgroup.
// One kernel, prc_walk_kernel: 122 VGPRs, no spill, no scratch, no LDS (tests/test_pr_metrics.py holds it within 128 from the code object).
#include "metrics_common.h"
#include "../../include/ecgvit_hip_pr.h"

static_assert(ECGVIT_PR_MAX_WEIGHT == (1 << 30) && ECGVIT_PR_SLOTS == 6, "weights in 30 bits");

// floor(a 2^32 / d) for a < 2^60, 0 < d < 2^30: a = qa d + ra gives a 2^32 / d = qa 2^32 + ra 2^32 / d, and the second term is below 2^32.
// Integer divisions only: an f64 quotient is wrong once a >= 2^53.
__device__ __forceinline__ uint64_t prc_term(uint64_t a, uint32_t d) {
    const uint64_t qa = a / d, ra = a - qa * d;
    return (qa << 32) + (ra << 32) / d;
}

// F(tp, fp) > F(bt, bf) under the class weight wp, by cross-multiplication: every factor is below 2^31 and 2^30
__device__ __forceinline__ int prc_cmp(uint32_t tp, uint32_t fp, uint32_t bt, uint32_t bf, uint32_t wp) {
    const uint64_t x = (uint64_t)tp * ((uint64_t)bt + bf + wp), y = (uint64_t)bt * ((uint64_t)tp + fp + wp);
    return x > y ? 1 : x < y ? -1 : 0;
}

// The walk skeleton is metrics_common.h's, as for rank_walk_kernel.
// Pass 1, the whole row in any order: wp / wn per replicate (the NaN-keyed records included).  F needs wp at its first comparison.
// Pass 2, positions first_nan[c] - 1 .. 0 in steps of ECGVIT_RANK_WALK_ROWS, lane l holding the V = 4 consecutive positions hi - 4 l - j: lane 0
// comes first in the walk.  Position p closes its group when p == 0 or the word at p - 1 carries the last-of-group bit: a lane reads V + 1 words,
// and a word below position 0 reads as a bare last-of-group bit.  State per replicate: wave-uniform TP, FP (the running sums) and TPc (TP at the last
// closing position); per lane, the u64 partial of ap_q and the best (tp, fp, position) among the lane's own closing positions.  A lane sums its
// positions, one exclusive wave scan per sum places it, TP at the closing before the lane comes from the highest lower lane that closed a group (a
// shuffle) or from the carry; a second pass over the lane's positions forms the terms.  A group that adds no positive weight has neither a term nor
// a chance at the maximum (the group before it has the same TP and no more FP, and comes first): both sit behind dTP > 0.
__global__ __launch_bounds__(WALK_THREADS) void prc_walk_kernel(const uint32_t *__restrict__ packed, const int32_t *__restrict__ first_nan, int64_t n, int K,
                                                                const uint32_t *__restrict__ mult, int64_t R, long long *__restrict__ out) {
    constexpr int G = ECGVIT_RANK_GROUP, V = ECGVIT_RANK_WALK_ROWS / WAVE;
    static_assert(V == 4, "four positions per lane");
    const WalkWave wv(packed, n, R);
    if (wv.r0 >= R) return;   // wave-uniform; the kernel holds no barrier
    const int l = wv.l;
    int64_t nan0 = first_nan[wv.c];
    nan0 = nan0 < 0 ? 0 : nan0 > n ? n : nan0;

    uint32_t wp[G], wn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) wp[g] = wn[g] = 0u;
    for (int64_t b = 0; b < n; b += ECGVIT_RANK_WALK_ROWS) {
        const int64_t p0 = b + (int64_t)l * V;
        uint32_t word[V];
#pragma unroll
        for (int j = 0; j < V; ++j) word[j] = p0 + j < n ? wv.order[p0 + j] : 0u;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            uint32_t w[G];
            walk_weights(wv, word[j], p0 + j < n, n, mult, R, w);
            const bool pos = word[j] & RANK_LABEL_BIT;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                wp[g] += pos ? w[g] : 0u;
                wn[g] += pos ? 0u : w[g];
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) wp[g] = walk_sum(wp[g]), wn[g] = walk_sum(wn[g]);

    uint32_t TP[G], FP[G], TPc[G], bt[G], bf[G];
    int32_t bp[G];
    uint64_t acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) TP[g] = FP[g] = TPc[g] = bt[g] = bf[g] = 0u, bp[g] = -1, acc[g] = 0ull;
    for (int64_t hi = nan0 - 1; hi >= 0; hi -= ECGVIT_RANK_WALK_ROWS) {
        const int64_t p0 = hi - (int64_t)l * V;   // the lane's highest position; its others are p0 - j
        uint32_t word[V + 1], w[V][G];
#pragma unroll
        for (int j = 0; j <= V; ++j) word[j] = p0 - j >= 0 ? wv.order[p0 - j] : j ? RANK_LAST_BIT : 0u;   // (word[0] below position 0: the lane holds nothing)
#pragma unroll
        for (int j = 0; j < V; ++j) walk_weights(wv, word[j], p0 - j >= 0, n, mult, R, w[j]);
        bool cl[V], any = false;
#pragma unroll
        for (int j = 0; j < V; ++j) cl[j] = p0 - j >= 0 && (word[j + 1] & RANK_LAST_BIT) != 0, any |= cl[j];
        const WalkCloses k = walk_closes(any, wv.below);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            uint32_t sp = 0, sa = 0, cp = 0;   // the lane's sums, and the positives' at its last closing position
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool pos = word[j] & RANK_LABEL_BIT;
                sp += pos ? w[j][g] : 0u;
                sa += pos ? 0u : w[j][g];
                if (cl[j]) cp = sp;
            }
            const uint32_t tp_in = TP[g] + walk_scan(sp, l) - sp, fp_in = FP[g] + walk_scan(sa, l) - sa;   // the sums before the lane
            const uint32_t tp_cl = tp_in + cp;
            const uint32_t tp_sh = __shfl(tp_cl, k.prev, WAVE);
            uint32_t tpc = k.before ? tp_sh : TPc[g], tp = tp_in, fp = fp_in;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool pos = word[j] & RANK_LABEL_BIT;
                tp += pos ? w[j][g] : 0u;
                fp += pos ? 0u : w[j][g];
                if (cl[j]) {
                    if (tp != tpc) {
                        acc[g] += prc_term((uint64_t)(tp - tpc) * tp, tp + fp);
                        if (prc_cmp(tp, fp, bt[g], bf[g], wp[g]) > 0) bt[g] = tp, bf[g] = fp, bp[g] = (int32_t)(p0 - j);
                    }
                    tpc = tp;
                }
            }
            const uint32_t tp_top = __shfl(tp_cl, k.top, WAVE);
            if (k.closes) TPc[g] = tp_top;
            TP[g] = __shfl(tp_in + sp, 63, WAVE), FP[g] = __shfl(fp_in + sa, 63, WAVE);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint64_t ap_q = walk_sum(acc[g]);
        uint32_t t = bt[g], f = bf[g];
        int32_t p = bp[g];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {   // larger F, then larger position: every lane ends with the same triple
            const uint32_t t2 = __shfl_xor(t, o, WAVE), f2 = __shfl_xor(f, o, WAVE);
            const int32_t p2 = __shfl_xor(p, o, WAVE);
            const int s = prc_cmp(t2, f2, t, f, wp[g]);
            if (s > 0 || (s == 0 && p2 > p)) t = t2, f = f2, p = p2;
        }
        if (l == 0 && wv.r0 + g < R) {
            long long *o = out + ((wv.r0 + g) * K + wv.c) * ECGVIT_PR_SLOTS;
            o[0] = (long long)ap_q, o[1] = (long long)wp[g], o[2] = (long long)wn[g];
            o[3] = (long long)t, o[4] = (long long)f, o[5] = (long long)p;
        }
    }
}

extern "C" int ecgvit_pr_walk(const uint32_t *packed, const int32_t *first_nan, int64_t n, int K, const uint32_t *mult, int64_t R, int64_t *out, void *stream) {
    if (!walk_args_ok(packed, first_nan, n, K, mult, R, out)) return ECGVIT_EINVAL;
    prc_walk_kernel<<<walk_grid(R, K), WALK_THREADS, 0, as_stream(stream)>>>(packed, first_nan, n, K, mult, R, reinterpret_cast<long long *>(out));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
