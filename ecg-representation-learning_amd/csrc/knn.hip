// Exact k-nearest-neighbour search over pooled representations, the merge of partial lists, the cosine metric's row normalisation and the
// weighted vote of a k-NN probe.  Contract, total order and the order of every sum: include/ecgvit_hip_knn.h.
#include "common.h"
#include "../../include/ecgvit_hip_knn.h"

#define KNN_THREADS 256
#define KNN_T ECGVIT_KNN_TILE     // queries and bank rows per score tile
#define KNN_KC 32                 // columns of d per LDS chunk
#define KNN_LD (KNN_KC + 1)       // operand row pitch in LDS: lane j reads row j, 33 j mod 64 is a different bank for every j
#define KNN_HALF (KNN_T / 2)      // bank rows of a tile that pass through LDS at once (the rows of one wave row)
#define KNN_SLD (KNN_HALF + 1)    // score row pitch in LDS: owner thread q reads row q
#define KNN_ROWS (KNN_T * KNN_KC / KNN_THREADS)   // operand elements per thread, chunk and operand (16)
#define KNN_LK 32                 // k up to which the lists of a workgroup live in LDS, one pair per lane (knn_search_kernel<true>)

// (s, n) stands before (ts, tn) under the total order: score descending, bank index ascending
template <typename I> __device__ __forceinline__ bool knn_before(float s, I n, float ts, I tn) { return s > ts || (s == ts && n < tn); }
__device__ __forceinline__ bool knn_finite(float s) { return fabsf(s) < __builtin_inff(); }   // false for NaN
__device__ __forceinline__ int64_t knn_shfl_xor(int64_t v, int o) {
    const int lo = __shfl_xor((int)(uint32_t)(uint64_t)v, o, 64), hi = __shfl_xor((int)(uint32_t)((uint64_t)v >> 32), o, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// =====================================================================================================
// search.  Workgroup (x, y) takes queries [128 x, 128 x + 128) against the bank tiles of row range y.  D = A . B + C on v_mfma_f32_32x32x2_f32
// with A = 32 bank rows (row i on lane i & 31, column 2 kk + (lane >> 5) of the chunk) and B = 32 queries (query j on lane j & 31, the same
// column): register g of lane (j, h) is the score of bank row (g & 3) + 8 (g >> 2) + 4 h of the MFMA tile for query j.  Wave (wr, wc) holds bank
// rows 64 wr .. 64 wr + 63 and queries 64 wc .. 64 wc + 63 of the tile as 2 x 2 accumulators; the chunks follow one another in ascending
// column order on the same accumulators, so each score is one fmaf chain over i = 0 .. d - 1.
// The next chunk's operands are loaded into registers before the current chunk's MFMAs and stored to LDS after them.
// After a tile the wave rows write their scores to LDS in turn (the operands' LDS, [query][bank row] with pitch 65).
// WL (k <= KNN_LK): the sorted list of (query, range) lives in LDS, pair j on lane j, and wave w owns queries 32 w .. 32 w + 31 of the tile.
// For each of them lane r compares score r with the list's k-th pair: one comparison per score, and a ballot that is empty for most queries
// once the lists have filled.  The queries with a winner are taken up again: the list goes to registers (one pair per lane), the winners are
// inserted in ascending bank row -- a ballot counts the pairs that stand before the winner, the lanes from there shift up by one -- and after
// each the k-th pair is broadcast and the remaining winners are compared again.  Empty slots hold (-inf, INT_MAX): behind every finite score.
// !WL: thread q < 128, the owner of query q, walks its 64 scores in ascending bank row: one comparison against (ts, tn), the list's k-th
// pair in registers, and on the rare win an insertion into the sorted list of (query, range) in the workspace, which only this thread
// reads or writes.
// =====================================================================================================
template <bool WL>
__global__ __launch_bounds__(KNN_THREADS, 2) void knn_search_kernel(const float *__restrict__ queries, int64_t ldq, const float *__restrict__ bank,
                                                                 int64_t ldb, int64_t Q, int64_t N, int d, int k, int64_t self_base, int S,
                                                                 float *ws_s, int64_t *ws_i) {
    __shared__ __attribute__((aligned(16))) float lds[2 * KNN_T * KNN_LD];
    __shared__ float lst_s[WL ? KNN_T * KNN_LK : 1];
    __shared__ int lst_n[WL ? KNN_T * KNN_LK : 1];
    float *sa = lds, *sb = lds + KNN_T * KNN_LD, *sc = lds;   // sc (128 x 65) fits in the two operand tiles (2 x 128 x 33)
    if (WL) {
        for (int e = threadIdx.x; e < KNN_T * KNN_LK; e += KNN_THREADS) {   // (each wave reads its own queries' lists only after a barrier)
            lst_s[e] = -__builtin_inff();
            lst_n[e] = 0x7fffffff;
        }
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;
    const int64_t q0 = (int64_t)blockIdx.x * KNN_T;
    const int64_t NT = (N + KNN_T - 1) / KNN_T;
    const int64_t t_lo = NT * blockIdx.y / S, t_hi = NT * (blockIdx.y + 1) / S;
    // the owner's list and its threshold
    const int64_t oq = q0 + tid;
    const bool owner = tid < KNN_T && oq < Q;
    float *ls = ws_s + ((int64_t)blockIdx.y * Q + (owner ? oq : 0)) * k;
    int64_t *li = ws_i + ((int64_t)blockIdx.y * Q + (owner ? oq : 0)) * k;
    const int64_t self = self_base >= 0 ? self_base + oq : -1;
    int cnt = 0;
    float ts = -__builtin_inff();
    int64_t tn = -1;
    // staging: thread (sr, sk) moves column sk of rows sr, sr + 8, ... of either operand
    const int sk = tid & 31, sr = tid >> 5;
    float va[KNN_ROWS], vb[KNN_ROWS];
    // Rows past N and queries past Q are read from the last valid row instead (their scores are never looked at, and no score depends on
    // another row's operand); columns past d are read from column d - 1 and replaced by zero, for both operands.
    const int last_q = (Q - q0 < KNN_T ? (int)(Q - q0) : KNN_T) - 1;
    auto load = [&](int64_t n0, int kc) {
        const bool kin = kc + sk < d;
        const int col = kin ? kc + sk : d - 1;
        const int last_a = (N - n0 < KNN_T ? (int)(N - n0) : KNN_T) - 1;
        const float *ga = bank + n0 * ldb + col, *gq = queries + q0 * ldq + col;
#pragma unroll
        for (int i = 0; i < KNN_ROWS; ++i) {
            const int ra = sr + 8 * i < last_a ? sr + 8 * i : last_a, rq = sr + 8 * i < last_q ? sr + 8 * i : last_q;
            const float a = ga[(uint32_t)ra * (uint32_t)ldb], b = gq[(uint32_t)rq * (uint32_t)ldq];   // (pitches below 2^24: the offset fits 32 bits)
            va[i] = kin ? a : 0.f;
            vb[i] = kin ? b : 0.f;
        }
    };
    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t n0 = t * KNN_T;
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.f;
        load(n0, 0);
        for (int kc = 0; kc < d; kc += KNN_KC) {
            __syncthreads();   // the previous chunk's operands, or the previous tile's scores, have been read
#pragma unroll
            for (int i = 0; i < KNN_ROWS; ++i) {
                sa[(sr + 8 * i) * KNN_LD + sk] = va[i];
                sb[(sr + 8 * i) * KNN_LD + sk] = vb[i];
            }
            __syncthreads();
            if (kc + KNN_KC < d) load(n0, kc + KNN_KC);
            const float *pa = sa + (wr * 64 + j) * KNN_LD + h, *pb = sb + (wc * 64 + j) * KNN_LD + h;
#pragma unroll 4
            for (int kk = 0; kk < KNN_KC / 2; ++kk) {
                const float a0 = pa[2 * kk], a1 = pa[32 * KNN_LD + 2 * kk], b0 = pb[2 * kk], b1 = pb[32 * KNN_LD + 2 * kk];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();   // the operands, or the other wave row's scores, have been read
            if (wr == pass) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
#pragma unroll
                        for (int g = 0; g < 16; ++g)
                            sc[(wc * 64 + b * 32 + j) * KNN_SLD + a * 32 + (g & 3) + 8 * (g >> 2) + 4 * h] = acc[a][b][g];
            }
            __syncthreads();
            const int64_t base = n0 + pass * KNN_HALF;
            const int lim = N - base < KNN_HALF ? (int)(N - base) : KNN_HALF;   // (<= 0: the whole half is past the bank)
            if (WL) {
                const int n = (int)base + lane;   // (N <= 2^31 - 128)
                const int nq = Q - q0 - wave * 32 < 32 ? (int)(Q - q0 - wave * 32) : 32;   // this wave's queries (<= 0: none)
                const int64_t self0 = self_base >= 0 ? self_base + q0 + wave * 32 : -1;
                uint32_t hits = 0;
#pragma unroll 8
                for (int u = 0; u < 32; ++u) {
                    const int ql = wave * 32 + u;
                    const float s = sc[ql * KNN_SLD + lane];
                    const float ts = lst_s[ql * KNN_LK + k - 1];
                    const int tn = lst_n[ql * KNN_LK + k - 1];
                    const bool c = lane < lim && u < nq && knn_finite(s) && (self0 < 0 || n != self0 + u) && knn_before(s, n, ts, tn);
                    if (__ballot(c)) hits |= 1u << u;
                }
                while (hits) {
                    const int u = __ffs(hits) - 1, ql = wave * 32 + u;
                    hits &= hits - 1;
                    const float s = sc[ql * KNN_SLD + lane];
                    float ls_ = -__builtin_inff();
                    int ln_ = 0x7fffffff;
                    if (lane < KNN_LK) {
                        ls_ = lst_s[ql * KNN_LK + lane];
                        ln_ = lst_n[ql * KNN_LK + lane];
                    }
                    float ts = __shfl(ls_, k - 1, 64);
                    int tn = __shfl(ln_, k - 1, 64);
                    bool c = lane < lim && knn_finite(s) && (self0 < 0 || n != self0 + u) && knn_before(s, n, ts, tn);
                    uint64_t mask = __ballot(c);
                    while (mask) {
                        const int l = __ffsll((unsigned long long)mask) - 1;
                        const float cs = __shfl(s, l, 64);
                        const int cn = (int)base + l;
                        const int pos = __popcll(__ballot(lane < k && knn_before(ls_, ln_, cs, cn)));   // (< k: the winner stands before pair k - 1)
                        const float up_s = __shfl_up(ls_, 1, 64);
                        const int up_n = __shfl_up(ln_, 1, 64);
                        if (lane == pos) {
                            ls_ = cs;
                            ln_ = cn;
                        } else if (lane > pos && lane < k) {
                            ls_ = up_s;
                            ln_ = up_n;
                        }
                        ts = __shfl(ls_, k - 1, 64);
                        tn = __shfl(ln_, k - 1, 64);
                        c = c && knn_before(s, n, ts, tn);
                        mask = __ballot(c) & ~((2ull << l) - 1ull);   // the winners after row l that still win
                    }
                    if (lane < k) {
                        lst_s[ql * KNN_LK + lane] = ls_;
                        lst_n[ql * KNN_LK + lane] = ln_;
                    }
                }
            } else if (owner) {
                for (int r = 0; r < lim; ++r) {
                    const float s = sc[tid * KNN_SLD + r];
                    const int64_t n = base + r;
                    if (!knn_finite(s) || n == self || (cnt == k && !knn_before(s, n, ts, tn))) continue;
                    int p = cnt < k ? cnt : k - 1;
                    while (p > 0) {
                        const float ps = ls[p - 1];
                        const int64_t pn = li[p - 1];
                        if (!knn_before(s, n, ps, pn)) break;
                        ls[p] = ps;
                        li[p] = pn;
                        --p;
                    }
                    ls[p] = s;
                    li[p] = n;
                    if (cnt < k) ++cnt;
                    if (cnt == k) {
                        ts = ls[k - 1];
                        tn = li[k - 1];
                    }
                }
            }
        }
    }
    if (WL) {   // (the wave's own lists: no barrier)
        for (int u = 0; u < 32 && q0 + wave * 32 + u < Q; ++u) {
            const int ql = wave * 32 + u;
            if (lane < k) {
                const float s = lst_s[ql * KNN_LK + lane];
                const int64_t at = ((int64_t)blockIdx.y * Q + q0 + ql) * k + lane;
                ws_s[at] = s;
                ws_i[at] = knn_finite(s) ? (int64_t)lst_n[ql * KNN_LK + lane] : -1;
            }
        }
    } else if (owner) {
        for (int p = cnt; p < k; ++p) {
            ls[p] = -__builtin_inff();
            li[p] = -1;
        }
    }
}

// =====================================================================================================
// merge: one wave per query.  Slot by slot, the first pair under the total order that stands strictly after the pair taken last: every lane
// sweeps its share of the P k_p entries, a butterfly leaves the winner on every lane.  No order of the input is assumed and a pair that
// stands twice is taken once.  R > 0: at most 64 R entries per query, read once into R registers per lane (an unusable entry as index -1);
// R = 0: any number, read again in every sweep.
// =====================================================================================================
#define KNN_MERGE_R 32
template <int R>
__global__ __launch_bounds__(KNN_THREADS) void knn_merge_kernel(const float *__restrict__ si, const int64_t *__restrict__ ii, int P, int64_t list_stride,
                                                                int64_t ld_in, int64_t Q, int kp, int k, int64_t index_base, float *__restrict__ so,
                                                                int64_t *__restrict__ io) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (KNN_THREADS / WAVE) + (threadIdx.x >> 6);
    if (q >= Q) return;   // (the whole wave; no barrier follows)
    const int M = P * kp;
    float es[R > 0 ? R : 1];
    int64_t en[R > 0 ? R : 1];
    if constexpr (R > 0) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int e = lane + WAVE * i;
            es[i] = -__builtin_inff();
            en[i] = -1;
            if (e < M) {
                const int p = e / kp, c = e - p * kp;
                const int64_t at = p * list_stride + q * ld_in + c;
                const float s = si[at];
                const int64_t n = ii[at];
                if (n >= 0 && knn_finite(s)) {
                    es[i] = s;
                    en[i] = n;
                }
            }
        }
    }
    float last_s = __builtin_inff();   // before every finite score
    int64_t last_n = -1;
    int slot = 0;
    for (; slot < k; ++slot) {
        float bs = -__builtin_inff();
        int64_t bn = -1;
        if constexpr (R > 0) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                if (en[i] >= 0 && knn_before(last_s, last_n, es[i], en[i]) && (bn < 0 || knn_before(es[i], en[i], bs, bn))) {
                    bs = es[i];
                    bn = en[i];
                }
            }
        } else {
            for (int e = lane; e < M; e += WAVE) {
                const int p = e / kp, c = e - p * kp;
                const int64_t at = p * list_stride + q * ld_in + c;
                const float s = si[at];
                const int64_t n = ii[at];
                if (n >= 0 && knn_finite(s) && knn_before(last_s, last_n, s, n) && (bn < 0 || knn_before(s, n, bs, bn))) {
                    bs = s;
                    bn = n;
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(bs, o, 64);
            const int64_t on = knn_shfl_xor(bn, o);
            if (on >= 0 && (bn < 0 || knn_before(os, on, bs, bn))) {
                bs = os;
                bn = on;
            }
        }
        if (bn < 0) break;   // (the same on every lane)
        if (lane == 0) {
            so[q * k + slot] = bs;
            io[q * k + slot] = bn + index_base;
        }
        last_s = bs;
        last_n = bn;
    }
    for (int p = slot + lane; p < k; p += WAVE) {
        so[q * k + p] = -__builtin_inff();
        io[q * k + p] = -1;
    }
}

// =====================================================================================================
// normalize: one wave per row, the sum of squares and the scaling in f64
// =====================================================================================================
__global__ __launch_bounds__(KNN_THREADS) void knn_normalize_kernel(const float *__restrict__ x, int64_t ldx, float *__restrict__ out, int64_t ldo,
                                                                    int64_t rows, int d) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (KNN_THREADS / WAVE) + (threadIdx.x >> 6);
    if (r >= rows) return;
    double sum = 0.0;
    for (int i = lane; i < d; i += WAVE) {
        const double v = (double)x[r * ldx + i];
        sum += v * v;   // (exact product: 48 bits)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const double inv = sum == 0.0 ? 0.0 : 1.0 / sqrt(sum);
    for (int i = lane; i < d; i += WAVE) out[r * ldo + i] = (float)((double)x[r * ldx + i] * inv);
}

// =====================================================================================================
// vote: one workgroup per query.  The weights once into LDS, then one thread per label column sums over the slots in ascending order.
// =====================================================================================================
__global__ __launch_bounds__(KNN_THREADS) void knn_vote_kernel(const float *__restrict__ scores, const int64_t *__restrict__ indices, int k,
                                                               const float *__restrict__ labels, int64_t ldy, int64_t N, int K, int mode,
                                                               double temperature, float *__restrict__ out) {
    __shared__ double w[ECGVIT_KNN_MAX_K];
    __shared__ int64_t id[ECGVIT_KNN_MAX_K];
    __shared__ float sv[ECGVIT_KNN_MAX_K];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    if (tid < k) {
        const int64_t n = indices[q * k + tid];
        id[tid] = n >= 0 && n < N ? n : -1;
        sv[tid] = scores[q * k + tid];
    }
    __syncthreads();
    if (tid < k) {
        double wt = 0.0;
        if (id[tid] >= 0) {
            wt = 1.0;
            if (mode == ECGVIT_KNN_VOTE_SOFTMAX) {
                float s0 = -__builtin_inff();
                for (int jj = 0; jj < k; ++jj)
                    if (id[jj] >= 0 && sv[jj] > s0) s0 = sv[jj];
                wt = exp(((double)sv[tid] - (double)s0) / temperature);
            }
        }
        w[tid] = wt;
    }
    __syncthreads();
    for (int c = tid; c < K; c += KNN_THREADS) {
        double num = 0.0, den = 0.0;
        bool any = false;
        for (int jj = 0; jj < k; ++jj) {
            if (id[jj] < 0) continue;
            any = true;
            num = __dadd_rn(num, __dmul_rn(w[jj], (double)labels[id[jj] * ldy + c]));
            den = __dadd_rn(den, w[jj]);
        }
        out[q * K + c] = any ? (float)(num / den) : 0.f;
    }
}

// =====================================================================================================
// host side
// =====================================================================================================
static int knn_splits(int64_t Q, int64_t N, int splits) {
    if (Q < 1 || N < 1 || splits < 0 || splits > ECGVIT_KNN_MAX_SPLITS) return 0;
    const int64_t NT = (N + KNN_T - 1) / KNN_T, QT = (Q + KNN_T - 1) / KNN_T;
    int64_t S = splits;
    if (S == 0) {   // at most two workgroups for each of 256 CUs (one more would run after all the others), at most 64 lists per query
        S = 512 / QT;
        if (S > 64) S = 64;
        if (S < 1) S = 1;
    }
    if (S > NT) S = NT;
    return (int)S;
}

static bool knn_search_args(int64_t Q, int64_t N, int d, int k, int64_t self_base) {
    if (Q < 1 || N < 1 || d < 1 || d > ECGVIT_ROW_MAX_D || k < 1 || k > ECGVIT_KNN_MAX_K || self_base < -1) return false;
    if (Q > ((int64_t)1 << 31) * KNN_T - KNN_T || N > ECGVIT_KNN_MAX_ROWS) return false;   // the grid's x extent; a row index in 32 bits
    return k <= (self_base < 0 ? N : N - 1);
}

static int64_t knn_score_bytes(int64_t Q, int S, int k) { return (Q * S * k * 4 + 15) / 16 * 16; }

extern "C" int ecgvit_knn_splits(int64_t Q, int64_t N, int splits) { return knn_splits(Q, N, splits); }

extern "C" int64_t ecgvit_knn_workspace(int64_t Q, int64_t N, int d, int k, int splits) {
    const int S = knn_splits(Q, N, splits);
    if (S == 0 || d < 1 || d > ECGVIT_ROW_MAX_D || k < 1 || k > ECGVIT_KNN_MAX_K) return 0;
    return knn_score_bytes(Q, S, k) + Q * S * k * 8;
}

static int knn_merge_launch(const float *si, const int64_t *ii, int P, int64_t list_stride, int64_t ld_in, int64_t Q, int kp, int k,
                            int64_t index_base, float *so, int64_t *io, void *stream) {
    const int per = KNN_THREADS / WAVE;
    const dim3 grid((unsigned)((Q + per - 1) / per));
    if ((int64_t)P * kp <= WAVE * KNN_MERGE_R)
        hipLaunchKernelGGL(knn_merge_kernel<KNN_MERGE_R>, grid, dim3(KNN_THREADS), 0, as_stream(stream), si, ii, P, list_stride, ld_in, Q, kp, k, index_base, so, io);
    else
        hipLaunchKernelGGL(knn_merge_kernel<0>, grid, dim3(KNN_THREADS), 0, as_stream(stream), si, ii, P, list_stride, ld_in, Q, kp, k, index_base, so, io);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

extern "C" int ecgvit_knn_search(const float *queries, int64_t ldq, const float *bank, int64_t ldb, int64_t Q, int64_t N, int d, int k,
                                 int64_t self_base, int64_t index_base, int splits, float *scores, int64_t *indices, void *workspace, void *stream) {
    const int S = knn_splits(Q, N, splits);
    if (S == 0 || !knn_search_args(Q, N, d, k, self_base) || ldq < d || ldb < d || ldq > ECGVIT_KNN_MAX_PITCH || ldb > ECGVIT_KNN_MAX_PITCH) return ECGVIT_EINVAL;
    if (!queries || !bank || !scores || !indices || !workspace || ((uintptr_t)workspace & 7)) return ECGVIT_EINVAL;
    float *ws_s = reinterpret_cast<float *>(workspace);
    int64_t *ws_i = reinterpret_cast<int64_t *>(reinterpret_cast<char *>(workspace) + knn_score_bytes(Q, S, k));
    const dim3 grid((unsigned)((Q + KNN_T - 1) / KNN_T), (unsigned)S);
    if (k <= KNN_LK)
        hipLaunchKernelGGL(knn_search_kernel<true>, grid, dim3(KNN_THREADS), 0, as_stream(stream), queries, ldq, bank, ldb, Q, N, d, k, self_base, S, ws_s, ws_i);
    else
        hipLaunchKernelGGL(knn_search_kernel<false>, grid, dim3(KNN_THREADS), 0, as_stream(stream), queries, ldq, bank, ldb, Q, N, d, k, self_base, S, ws_s, ws_i);
    ECGVIT_CHECK_LAUNCH();
    return knn_merge_launch(ws_s, ws_i, S, Q * k, k, Q, k, k, index_base, scores, indices, stream);
}

extern "C" int ecgvit_knn_merge(const float *scores_in, const int64_t *indices_in, int P, int64_t list_stride, int64_t ld_in, int64_t Q, int k_p, int k,
                                int64_t index_base, float *scores, int64_t *indices, void *stream) {
    if (P < 1 || k_p < 1 || (int64_t)P * k_p > ECGVIT_KNN_MAX_MERGE || k < 1 || k > ECGVIT_KNN_MAX_K || ld_in < k_p || Q < 1 || list_stride < 0)
        return ECGVIT_EINVAL;
    if (Q > ((int64_t)1 << 31)) return ECGVIT_EINVAL;
    if (!scores_in || !indices_in || !scores || !indices) return ECGVIT_EINVAL;
    return knn_merge_launch(scores_in, indices_in, P, list_stride, ld_in, Q, k_p, k, index_base, scores, indices, stream);
}

extern "C" int ecgvit_knn_normalize(const float *x, int64_t ldx, float *out, int64_t ldo, int64_t rows, int d, void *stream) {
    if (rows < 1 || rows > ((int64_t)1 << 31) || d < 1 || d > ECGVIT_ROW_MAX_D || ldx < d || ldo < d || !x || !out) return ECGVIT_EINVAL;
    const int per = KNN_THREADS / WAVE;
    hipLaunchKernelGGL(knn_normalize_kernel, dim3((unsigned)((rows + per - 1) / per)), dim3(KNN_THREADS), 0, as_stream(stream), x, ldx, out, ldo, rows, d);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

extern "C" int ecgvit_knn_vote(const float *scores, const int64_t *indices, int64_t Q, int k, const float *labels, int64_t ldy, int64_t N, int K,
                               int mode, double temperature, float *out, void *stream) {
    if (Q < 1 || Q >= ((int64_t)1 << 31) || N < 1 || k < 1 || k > ECGVIT_KNN_MAX_K || K < 1 || K > ECGVIT_KNN_MAX_CLASSES || ldy < K) return ECGVIT_EINVAL;
    if (mode != ECGVIT_KNN_VOTE_UNIFORM && mode != ECGVIT_KNN_VOTE_SOFTMAX) return ECGVIT_EINVAL;
    if (mode == ECGVIT_KNN_VOTE_SOFTMAX && !(temperature > 0.0 && temperature < __builtin_inf())) return ECGVIT_EINVAL;
    if (!scores || !indices || !labels || !out) return ECGVIT_EINVAL;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)Q), dim3(KNN_THREADS), 0, as_stream(stream), scores, indices, k, labels, ldy, N, K, mode,
                       temperature, out);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
