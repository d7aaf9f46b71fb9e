/* Average precision and class-wise F-max on the sorted order of ecgvit_hip_rank.h: csrc/pr_metrics.hip, exported by libecgvit_hip.so and bound by a
 * table of its own (pr_abi.py).  The conventions are those of ecgvit_hip.h and ecgvit_hip_rank.h: a status return (ECGVIT_OK / ECGVIT_EINVAL /
 * ECGVIT_ELAUNCH), raw device pointers, `void *stream` last; the entry point validates every argument and returns ECGVIT_EINVAL before it launches
 * anything.  Additive: the ABI version stays 6.  Everything the device produces is an exact integer; no atomics, no floating point, no kernel that
 * waits for another workgroup.
 *
 * input    `packed` u32 (K, n) and `first_nan` int32 (K) as ecgvit_rank_sort leaves them (record index | label bit << 30 | last-of-tie-group
 *          bit << 31 per ascending sorted position); `mult` null, or u32 (n, R4) record-major as ecgvit_rank_multiplicities* leave it for the same
 *          R (R4 = R rounded up to a multiple of 4, 16-byte aligned).
 *
 * weights  for class c and replicate r every record carries an integer weight w: 1 everywhere when `mult` is null, else mult[i][r].
 *          wp / wn = the total weight of the positives / negatives of the class, the records with NaN's key included.
 *
 * walk     over the sorted positions below first_nan[c], DESCENDING (the highest score first), tie group by tie group.  A record with NaN's key is
 *          never predicted positive and still counts in wp / wn: the rule of the AUROC walk (a NaN compares false against every threshold).
 *          After group g, TP_g and FP_g are the cumulative positive and negative weight of groups 1..g (TP_0 = 0): the confusion counts at the
 *          threshold "score >= the group's score".
 *
 * average precision, as one integer
 *            ap_q = sum over groups g of floor( (TP_g - TP_{g-1}) * TP_g * 2^32 / (TP_g + FP_g) );   a group with TP_g == TP_{g-1} adds nothing
 *            AP   = ap_q / (2^32 * wp)
 *          This is the step-wise sum of (recall_g - recall_{g-1}) * precision_g -- scikit-learn's average_precision_score(y, s, sample_weight=w)
 *          -- with every term truncated to 2^-32 of a weight unit.  At most wp groups have a non-zero term, so 0 <= AP_exact - AP < 2^-32.  An
 *          exact integer is order-free: the result does not depend on the tiling and equals a restatement in unbounded integers bit for bit.
 *
 * class-wise F-max and its threshold
 *          over the same groups, the maximum of F_g = 2 TP_g / (TP_g + FP_g + wp), compared by cross-multiplication in 64-bit integers:
 *            F_a > F_b  <=>  TP_a * (TP_b + FP_b + wp) > TP_b * (TP_a + FP_a + wp)
 *          The start value is F = 0 with no group (pos = -1: predict nothing).  A group replaces the best only when strictly greater: ties go to
 *          the highest threshold, and a group of zero total weight is never chosen.  (f_tp, f_fp) = (TP_g, FP_g) of the winning group, f_pos = the
 *          ascending sorted position of its lowest member; the host reads the threshold as the score of record packed[c][f_pos] & 0x3FFFFFFF.
 *          wp == 0 gives (0, 0, -1).
 *
 * output   out int64 (R, K, ECGVIT_PR_SLOTS) dense = (ap_q, wp, wn, f_tp, f_fp, f_pos).  A class is valid in a replicate when wp > 0 and wn > 0
 *          (the reference's msk_2_class rule, as the AUROC route applies it); macro values are means over a replicate's valid classes.
 *
 * kernel   prc_walk_kernel, in the shape of rank_walk_kernel: a wave owns one class and ECGVIT_RANK_GROUP replicates; a workgroup is four waves.
 *          A first pass over the whole row sums wp / wn (F needs wp before the first comparison).  The walk then reads the row once from
 *          first_nan[c] - 1 down to 0, ECGVIT_RANK_WALK_ROWS positions per step, four consecutive ones per lane, gathers a record's multiplicities
 *          with one 16-byte load, sums a lane's positions in registers and places the lane with one wave scan per sum.  Walking down, a group
 *          closes at position p when p == 0 or the word at p - 1 carries bit 31; at a closing position the lane forms TP_g - TP_{g-1} against the
 *          running TP at the closing before it (from the highest earlier lane that closed a group, or the step's carry), adds the truncated term
 *          to its own u64 partial and compares the F candidate with its own best.  At the end of the row the partials are added and the bests
 *          reduced across the wave: larger F, then larger position.  The quotient is the exact floor, by two 64-bit integer divisions:
 *          a = qa d + ra, floor(a 2^32 / d) = (qa << 32) + floor((ra << 32) / d).
 *
 * limits   n, K, R as ecgvit_hip_rank.h: 1 <= n <= ECGVIT_RANK_MAX_ROWS, 1 <= K <= ECGVIT_RANK_MAX_CLASSES, 1 <= R <= ECGVIT_RANK_MAX_REPLICATES.
 *          The caller guarantees that the weights of a replicate sum to less than ECGVIT_PR_MAX_WEIGHT = 2^30 (a bootstrap replicate sums to n;
 *          unit weights to n).  Then (TP_g - TP_{g-1}) * TP_g < 2^60, ap_q <= 2^32 * wp < 2^62, and both sides of the F comparison stay below
 *          2^30 * 2^31 < 2^63.  The sum is not checked on the device. */
#ifndef ECGVIT_HIP_PR_H
#define ECGVIT_HIP_PR_H
#include "ecgvit_hip_rank.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECGVIT_PR_SLOTS 6                 /* int64 per (replicate, class): ap_q, wp, wn, f_tp, f_fp, f_pos */
#define ECGVIT_PR_MAX_WEIGHT 1073741824   /* the weights of one replicate sum to less than this (1 << 30) */

int ecgvit_pr_walk(const uint32_t *packed, const int32_t *first_nan, int64_t n, int K, const uint32_t *mult, int64_t R, int64_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
