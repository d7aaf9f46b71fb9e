/* Scalable k-means++ (k-means||; Bahmani, Moseley, Vattani, Kumar, Vassilvitskii, "Scalable K-Means++", VLDB 2012) seeding for the segment
 * tokenizer: csrc/tok_scalable.hip, exported by libecgvit_hip.so beside the entry points of ecgvit_hip.h and bound by a table of their own
 * (tok_scalable_abi.py).  The conventions are those of ecgvit_hip.h: a status return (ECGVIT_OK / ECGVIT_EINVAL / ECGVIT_ELAUNCH), raw device
 * pointers, a caller-owned workspace whose size query returns 0 when the arguments are unsupported, `void *stream` last.  Additive: the ABI
 * version stays 6.
 *
 * The reference's GPU route (models/ecg_tokenizer.py:29, backend='cuml') seeds with init='scalable-k-means++'.  What is built here is the
 * paper's algorithm under this project's integer rules, NOT cuML's random stream and not its exact variant: parity with cuML is UNPINNED
 * (cuML is not available to the tests), and the string 'scalable-k-means++' stays refused by tokenizer.py.
 *
 * The store, the segment index g = c * n_seg + p, a segment's bits s_g, the unfused f32 distance d2, the absolute maximum A, E, H, F and the
 * integer weight q(d2) = rint(d2 * 2^F) (0 for a non-finite distance) are exactly those of ecgvit_tok_seed (ecgvit_hip.h).
 *
 * inputs   V centres; ell = ceil(oversampling_factor * V) (formed by the caller); n_rounds = R rounds; n_trials = T local trials; `first`, a
 *          segment index; keys[R] (uint64, a HOST array); u0 and u53[(V - 1) * T] (device), each below 2^53; cap, the most rows a round appends
 *          (the caller's default: ell + 8 * ceil(sqrt(ell))).  1 + R * cap <= ECGVIT_TOK_MAX_CLUSTERS.
 * state    a candidate table whose row j holds the mean-removed bits of one segment, its g in cand_g[j]; closest(g) = +inf; owner(g) unset.
 *   1 fold       the rows appended since the last fold are folded in row order (before round 0: row 0, segment `first`).  For row j:
 *                d = d2(s_g, row_j); if d < closest(g) then closest(g) = d and owner(g) = j.  Strict: the smaller row wins a tie; a NaN
 *                distance changes nothing.
 *   2 potential  pot = sum_g q(closest(g)).  pot == 0 ends the rounds: no weight is positive, so nothing is selected from there on.
 *   3 select     u(g) = mix(keys[r], g) >> 11 with mix = splitmix64's finaliser of z = keys[r] + g * 0x9E3779B97F4A7C15 (mod 2^64):
 *                z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.  Segment g is selected iff
 *                q > 0 and ((u(g) * pot) >> 53) < ell * q, both sides taken from products wider than 64 bits: probability
 *                min(1, ell q / pot) per segment, independently; no sum order is involved.
 *   4 append     the selected segments are appended in ascending g, at most cap per round; the rest of the round is dropped and counted.
 *   5 weights    after the last round one more fold; then w_j = #{g : owner(g) = j} over the segments whose closest is finite.
 *   6 recluster  weighted greedy k-means++ over the n_c table rows with the rules of ecgvit_tok_seed step for step (T trials per centre, the
 *                target (U * pot) >> 53, the smallest row whose running sum exceeds it, the argmin of the potentials with ties to the smaller
 *                trial, row 0 when pot == 0), where every weight is w_j * q(d2(row_j, nearest chosen row)) with the same F (the sums stay
 *                below 2^63 because sum w <= C * n_seg), and centre 0 is the smallest j whose running sum of w exceeds (u0 * sum w) >> 53
 *                (j = 0 when sum w == 0).  centers (f32 [V][k]) = the chosen rows, indices (int64 [V]) = their cand_g.
 *   7            n_c < V: the recluster writes nothing; the caller reads info[0] and refuses.
 * Everything is enqueued on `stream` without a host read: the kernels take the row counts from `info`.  One launch for row 0, 5 per round
 * (fold, potential, count, scan, scatter), 4 after the last (fold, potential, weights, recluster).
 * No floating-point atomics; the only atomics are the integer additions of step 5.  The same arguments give the same bits, and a record
 * set gives the same result as a rectangle, a ragged store, an idxs subset and its compact copy.
 *
 * Kernels: the fold keeps ECGVIT_TOK_SEED_SPAN segments of one lead per workgroup in registers (four per thread), streams the new rows past
 * them through LDS in chunks of ECGVIT_TOK_SCALABLE_FOLD_ROWS, rewrites closest and owner (4 + 4 bytes read and written per segment) and leaves
 * one uint64 partial of sum q per workgroup; the selection counts per workgroup of ECGVIT_TOK_SCALABLE_SELECT_SPAN segments, scans the counts
 * in one workgroup and scatters (ascending g by construction, whatever the scheduling); the weights are a histogram of owner whose equal lanes
 * of a wave are added up before the one atomic; the recluster is one workgroup that walks all V centres in one launch. */
#ifndef ECGVIT_HIP_TOK_SCALABLE_H
#define ECGVIT_HIP_TOK_SCALABLE_H
#include "ecgvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECGVIT_TOK_SCALABLE_MAX_ROUNDS 16    /* n_rounds */
#define ECGVIT_TOK_SCALABLE_FOLD_ROWS 256    /* table rows per LDS chunk of the fold's row stream */
#define ECGVIT_TOK_SCALABLE_SELECT_SPAN 256  /* consecutive positions of one lead per workgroup of the selection */
#define ECGVIT_TOK_SCALABLE_INFO_HEAD 4      /* words of `info` before the per-round blocks */

/* bytes of `workspace`: the absolute maximum (16 bytes, as ecgvit_tok_seed keeps it), the candidate table (f32 [1 + R cap][k]), the recluster's
 * distances, the fold's partials, the selection's counts, closest (f32 [C n_seg]) and owner (int32 [C n_seg]).  0 when unsupported. */
int64_t ecgvit_tok_scalable_workspace(int C, int64_t n_seg, int V, int k, int n_trials, int n_rounds, int64_t cap);
/* cand_g (int64 [1 + R cap]) and weights (uint64 [1 + R cap]): the first info[0] entries are the candidates' segment indices and their weights.
 * info (uint64 [ECGVIT_TOK_SCALABLE_INFO_HEAD + 3 R + 1]): info[0] = n_c, info[1 .. 3] the kernels' own; then selected[R] (segments the rule took
 * in round r), truncated[R] (those of them that cap dropped), pots[R + 1] (the potential each round drew under; the last: after the final fold).
 * keep_amax == 1: the sweep for A is skipped and the maximum a previous call left in the first 16 bytes of this workspace is used again (the
 * same bytes ecgvit_tok_seed keeps there).  u53 may be NULL when V == 1. */
int ecgvit_tok_scalable_seed(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                             const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, int V, int n_trials,
                             int n_rounds, int64_t ell, int64_t cap, int64_t first, const uint64_t *keys, uint64_t u0, const uint64_t *u53,
                             float *centers, int64_t *indices, int64_t *cand_g, uint64_t *weights, uint64_t *info, void *workspace,
                             int keep_amax, void *stream);

#ifdef __cplusplus
}
#endif
#endif
