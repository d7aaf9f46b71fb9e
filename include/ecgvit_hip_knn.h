/* Exact k-nearest-neighbour search over pooled representations, and what a k-NN probe needs beside it: csrc/knn.hip, exported by
 * libecgvit_hip.so beside the entry points of ecgvit_hip.h and bound by a table of their own (knn_abi.py).  The conventions are those of
 * ecgvit_hip.h: a status return (ECGVIT_OK / ECGVIT_EINVAL / ECGVIT_ELAUNCH), raw device pointers, row pitches in elements, a caller-owned
 * workspace whose size query returns 0 when the arguments are unsupported, `void *stream` last.  Every entry point validates its arguments
 * and returns ECGVIT_EINVAL before it launches anything.  Additive: the ABI version stays 6.
 *
 * search   queries f32 (Q, d) with row pitch ldq, bank f32 (N, d) with row pitch ldb -> scores f32 (Q, k), indices int64 (Q, k), both dense.
 *   score    score[q][n] = the f32 fmaf chain over i = 0 .. d-1 of q[i] * b[i], started from 0: acc = fmaf(q[i], b[i], acc).  That is what
 *            v_mfma_f32_32x32x2_f32 gives over ascending i, so a score is the same bits whatever the tiling, the split or the batch.  (The
 *            tail of the last chunk of 32 is zero-filled: a chain that ends on -0 is reported as +0.)
 *   order    the result of query q is the first k admissible bank rows under the total order (score descending, bank index ascending), written
 *            in that order.  Every comparison of the kernels, the running threshold of a list included, is made under that total order on
 *            (score, index) pairs: the result does not depend on the order in which tiles, waves or splits meet a row.
 *   admissible  a row whose score is finite, and which is not the query's own (below).  A non-finite score never enters a list.  A query with
 *            fewer than k admissible rows gets index -1 and score -inf in the remaining slots.
 *   self_base   int64, -1 = none: query q never receives bank row self_base + q (leave-one-out for queries that are rows self_base ..
 *            self_base + Q - 1 of the bank).  By index, not by score: a twin of the excluded row is still returned.
 *   index_base  added to every reported index (not to -1).  self_base is in un-shifted bank rows.
 *   limits   1 <= d <= ECGVIT_ROW_MAX_D; 1 <= k <= ECGVIT_KNN_MAX_K; k <= N when self_base < 0, else k <= N - 1; Q >= 1; 1 <= N <= ECGVIT_KNN_MAX_ROWS; self_base >= -1;
 *            d <= ldq, ldb <= ECGVIT_KNN_MAX_PITCH; 0 <= splits <= ECGVIT_KNN_MAX_SPLITS.  Q * N may exceed 2^32.  Nothing past row Q / N or column d is read.
 *   memory   the (Q, N) matrix is never stored.  The bank is cut into S row ranges of whole tiles (S = ecgvit_knn_splits(Q, N, splits): the
 *            caller's value capped by the number of bank tiles; splits = 0: chosen so that a small Q still fills the device); workgroup
 *            (query tile, range) leaves one sorted list per query and range in the workspace, O(Q S k) bytes, and a second launch merges them.
 *   kernel   knn_search_kernel: a 128 x 128 score tile per workgroup of four waves (ECGVIT_KNN_TILE), 2 x 2 MFMA tiles of 32 x 32 per wave, d
 *            in chunks of 32 staged through LDS with tail rows, tail columns and the tail of d zero-filled; the bank rows are the A operand
 *            and the queries the B operand, so a lane's accumulators all belong to its own query columns.  The tile's scores pass through
 *            the same LDS to the selection: one comparison per score against the query's current k-th best pair, and an insertion for the
 *            rare winner -- for k <= 32 by a wave into a list kept in LDS, one pair per lane; above, by one owner thread per query into the
 *            list in the workspace.  No atomics, no spill, no scratch.
 *
 * merge    P lists of (Q, k_p) scores and indices, list p at scores_in + p * list_stride (elements; the same for indices_in) with row pitch
 *          ld_in -> the first k pairs under the same total order, dense (Q, k).  Slots with a negative index or a non-finite score are
 *          ignored; the lists need not be sorted; a pair that stands in several lists is reported once.  index_base is added to every
 *          reported index.  Fewer than k pairs: index -1, score -inf.  One wave per query, k selection sweeps (knn_merge_kernel).
 *          limits: P, k_p >= 1; P * k_p <= ECGVIT_KNN_MAX_MERGE; 1 <= k <= ECGVIT_KNN_MAX_K; ld_in >= k_p; Q >= 1.
 *
 * normalize  out[r][i] = fl32(x[r][i] * (1 / sqrt(sum_i x[r][i]^2))), the sum (over ascending i per lane, 64 lanes, then a butterfly) and the
 *          product in f64.  A zero row stays zero.  A non-finite row gives a non-finite row, which the search then never returns.
 *          limits: rows >= 1; 1 <= d <= ECGVIT_ROW_MAX_D; ldx, ldo >= d.
 *
 * vote     scores, indices dense (Q, k) as the search wrote them (un-shifted: index_base = 0), labels f32 (N, K) with row pitch ldy ->
 *          out[q][c] = sum_j w_j * y[idx_j][c] / sum_j w_j, dense (Q, K); the sums in f64 over j ascending, the quotient in f64, stored as f32.
 *          Slots whose index is outside [0, N) (-1 among them) are skipped; a query with no neighbour gets 0.
 *          mode ECGVIT_KNN_VOTE_UNIFORM: w_j = 1.  ECGVIT_KNN_VOTE_SOFTMAX: w_j = exp((s_j - s_0) / temperature) in f64, s_0 the largest score
 *          of the query's kept slots, so no weight exceeds 1; temperature > 0 and finite.
 *          limits: Q, N >= 1; 1 <= k <= ECGVIT_KNN_MAX_K; 1 <= K <= ECGVIT_KNN_MAX_CLASSES; ldy >= K. */
#ifndef ECGVIT_HIP_KNN_H
#define ECGVIT_HIP_KNN_H
#include "ecgvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECGVIT_KNN_MAX_K 256          /* neighbours per query */
#define ECGVIT_KNN_MAX_SPLITS 1024    /* row ranges of the bank */
#define ECGVIT_KNN_TILE 128           /* queries and bank rows per score tile */
#define ECGVIT_KNN_MAX_ROWS 2147483520 /* N of a search (2^31 - 128): a row index of the last tile fits 32 bits */
#define ECGVIT_KNN_MAX_PITCH 16777216 /* ldq, ldb of a search: an offset inside a tile fits 32 bits */
#define ECGVIT_KNN_MAX_MERGE 1048576  /* P * k_p of a merge */
#define ECGVIT_KNN_MAX_CLASSES 65536  /* label columns of a vote */
#define ECGVIT_KNN_VOTE_UNIFORM 0
#define ECGVIT_KNN_VOTE_SOFTMAX 1

/* the number of row ranges a search with these arguments cuts the bank into; 0 when unsupported */
int ecgvit_knn_splits(int64_t Q, int64_t N, int splits);
/* bytes of `workspace`: S lists of k (f32 score, int64 index) pairs per query.  0 when unsupported. */
int64_t ecgvit_knn_workspace(int64_t Q, int64_t N, int d, int k, int splits);
int ecgvit_knn_search(const float *queries, int64_t ldq, const float *bank, int64_t ldb, int64_t Q, int64_t N, int d, int k, int64_t self_base,
                      int64_t index_base, int splits, float *scores, int64_t *indices, void *workspace, void *stream);
int ecgvit_knn_merge(const float *scores_in, const int64_t *indices_in, int P, int64_t list_stride, int64_t ld_in, int64_t Q, int k_p, int k,
                     int64_t index_base, float *scores, int64_t *indices, void *stream);
int ecgvit_knn_normalize(const float *x, int64_t ldx, float *out, int64_t ldo, int64_t rows, int d, void *stream);
int ecgvit_knn_vote(const float *scores, const int64_t *indices, int64_t Q, int k, const float *labels, int64_t ldy, int64_t N, int K, int mode,
                    double temperature, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
