/* Rank-based AUROC and bootstrap replicates on the device: csrc/rank_metrics.hip, exported by libecgvit_hip.so beside the entry points of
 * ecgvit_hip.h and bound by a table of their own (rank_abi.py).  The conventions are those of ecgvit_hip.h: a status return (ECGVIT_OK /
 * ECGVIT_EINVAL / ECGVIT_ELAUNCH), raw device pointers, row pitches in elements, a caller-owned workspace whose size query returns 0 when the
 * arguments are unsupported, `void *stream` last.  Every entry point validates its arguments and returns ECGVIT_EINVAL before it launches
 * anything.  Additive: the ABI version stays 6.  Everything the device produces is an exact integer; no floating-point atomic, no kernel that
 * waits for another workgroup: launch boundaries are the only ordering between workgroups.
 *
 * key      score s of record i, class c -> p = s, or with from_logits the as_prob(s) of ecgvit_eval_counts (csrc/metrics_common.h: one
 *          definition).  NaN -> 0xFFFFFFFF.  Else p == 0 is taken as +0 (the float comparison ties -0 and +0), b = the bits of p, and
 *          key = b < 2^31 ? b | 0x80000000 : ~b.  key order = float order on everything that is not NaN; NaN is the largest key.
 *
 * sort     scores f32 (n, K) with row pitch ld, labels f32 (n, K) with row pitch ldl -> packed u32 (K, n) dense and first_nan int32 (K).
 *          Row c of `packed` is the permutation of the records under (key ascending, record index ascending), one word per sorted position:
 *            bits 0..29  the record index
 *            bit 30      the label bit, labels[i][c] != 0
 *            bit 31      set on the last position of its tie group (the next position holds another key, or there is none)
 *          first_nan[c] = the first sorted position whose key is NaN's; n when the class holds none.
 *          kernels  rank_keys_kernel reads the strided columns once, through an LDS transpose, into a (K, n) key plane; everything later is
 *                   coalesced or indexed inside one class row.  Then a stable least-significant-digit radix sort of (key, record index), four
 *                   passes of 8 bits, each of three launches over a grid of (tiles, classes): rank_hist_kernel (a 256-bin histogram per tile of
 *                   ECGVIT_RANK_TILE rows, integer LDS atomics), rank_scan_kernel (one workgroup per class: thread d runs over the tiles of
 *                   digit d, ECGVIT_RANK_SCAN_BATCH tiles per step, then the 256 digit totals) and rank_scatter_kernel (a wave owns a quarter
 *                   of the tile; a row's place among the rows of its digit comes from wave ballots, so the pass is stable).  rank_pack_kernel
 *                   marks the tie groups and gathers the label bits.
 *          limits   1 <= n <= ECGVIT_RANK_MAX_ROWS (two flag bits beside the index); 1 <= K <= ECGVIT_RANK_MAX_CLASSES (a grid dimension);
 *                   ld, ldl >= K.  workspace: ecgvit_rank_workspace(n, K, 0) bytes, 256-byte aligned.
 *
 * walk     the weighted rank sum.  For class c and replicate r with multiplicities w (`mult` as the replicates' entry points leave it for the same
 *          R; w = 1 everywhere when `mult` is null),
 *          Cn = the running sum of the negatives' weights over the sorted order:
 *            num2 = sum over positives t of w_t * (Cn[before t's tie group] + Cn[end of t's tie group]),  wp / wn = the positives' / negatives' weight.
 *          With w = 1, num2 is the integer ecgvit_eval_counts leaves in counts[4 + K + c]: the sum over (positive, negative) pairs of
 *          2 [p_i > p_j] + [p_i == p_j]; num2 / (2 wp wn) is the AUROC under sample weights w.  A record whose key is NaN's (position >=
 *          first_nan[c]) adds nothing to num2 and still counts in wp / wn: a NaN compares false against everything.
 *          out int64 (R, K, 3) dense = (num2, wp, wn).  pairs: null, or with R = 1 an int64 (K) that receives num2 as well (the pair slots of
 *          an ecgvit_eval_counts buffer).
 *          kernel   rank_walk_kernel: a wave reads the packed order of class c once, ECGVIT_RANK_WALK_ROWS positions per step (four
 *                   consecutive ones per lane), for ECGVIT_RANK_GROUP replicates; it gathers the replicates' multiplicities of a record
 *                   with one 16-byte load, sums a lane's positions in registers, takes one wave scan of the lanes' (positives, negatives) per replicate, and a lane
 *                   fetches the sums at the last closing position before it by a lane shuffle.  The carry from step to step is three
 *                   integers per replicate: Cn at the last closed tie group and the open group's positive and negative weight.  A workgroup
 *                   is four waves: 4 * ECGVIT_RANK_GROUP replicates of one class.
 *          limits   n, K as the sort; 1 <= R <= ECGVIT_RANK_MAX_REPLICATES per call.  n < 2^30 keeps Cn in 32 bits and num2 below 2^63.
 *
 * replicates   a replicate is a vector of multiplicities, u32 per record, that sums to n.  R of them lie record-major in the caller's workspace:
 *          mult u32 (n, R4) dense, R4 = R rounded up to a multiple of 4, mult[i][r] = the draws of record i in replicate r, the columns past R
 *          zero (ecgvit_rank_workspace(n, K, R) bytes, 16-byte aligned).  Record-major because the walk gathers by record index: the
 *          replicates of a wave share the fetched cache line.  Both entry points zero the buffer and count with integer atomics.
 *          indices  int64 (R, n) with row pitch ld, draws with replacement: mult[indices[r][j]][r] += 1.  A draw outside [0, n) is dropped
 *                   (nothing is written out of bounds; the replicate then sums to less than n).
 *          seed     draw j of replicate r (r counted from the first replicate of the whole run: `first` is the number of the chunk's first
 *                   row, so the draws do not depend on the chunking):
 *                     mix(z) = z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31   (mod 2^64)
 *                     key_r = mix(seed + 0x9E3779B97F4A7C15 * (r + 1));  u = mix(key_r + 0x9E3779B97F4A7C15 * (j + 1));  index = (u * n) >> 64
 *                   (the finaliser of SplitMix64; the multiply-shift map to [0, n) without rejection: an index is drawn with probability
 *                   floor-or-ceil(2^64 / n) / 2^64, a relative bias below n / 2^64 < 2^-34).  Two score sets evaluated with one seed are
 *                   resampled identically. */
#ifndef ECGVIT_HIP_RANK_H
#define ECGVIT_HIP_RANK_H
#include "ecgvit_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ECGVIT_RANK_TILE 2048             /* rows per workgroup of a sort pass */
#define ECGVIT_RANK_SCAN_BATCH 8          /* tiles per step of the scan over a digit's tiles */
#define ECGVIT_RANK_GROUP 4               /* replicates a wave of the walk carries beside each other */
#define ECGVIT_RANK_WALK_ROWS 256         /* sorted positions per step of a wave of the walk */
#define ECGVIT_RANK_MAX_ROWS 1073741824   /* n (1 << 30): a record index beside two flag bits */
#define ECGVIT_RANK_MAX_CLASSES 65535     /* K: a grid dimension */
#define ECGVIT_RANK_MAX_REPLICATES 1048576 /* R of one call */

/* bytes of `workspace`: R = 0, of a sort (two key planes, two index planes, the tile histograms, the digit bases); R >= 1, of the multiplicities
 * of R replicates.  0 when unsupported. */
int64_t ecgvit_rank_workspace(int64_t n, int K, int64_t R);
int ecgvit_rank_sort(const float *scores, int64_t ld, const float *labels, int64_t ldl, int64_t n, int K, int from_logits, uint32_t *packed,
                     int32_t *first_nan, void *workspace, void *stream);
int ecgvit_rank_multiplicities(const int64_t *indices, int64_t ld, int64_t R, int64_t n, uint32_t *mult, void *stream);
int ecgvit_rank_multiplicities_seeded(uint64_t seed, int64_t first, int64_t R, int64_t n, uint32_t *mult, void *stream);
int ecgvit_rank_walk(const uint32_t *packed, const int32_t *first_nan, int64_t n, int K, const uint32_t *mult, int64_t R, int64_t *out,
                     int64_t *pairs, void *stream);

#ifdef __cplusplus
}
#endif
#endif
