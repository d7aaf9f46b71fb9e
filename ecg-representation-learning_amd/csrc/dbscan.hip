// DBSCAN over the tokenizer's mean-removed segments (tokenizer.EcgTokenizer.dbscan; the reference's `dbscan` clustering, models/ecg_tokenizer.py,
// through sklearn).  Contract -- the segment order q, the neighbour rule on tok_d2, core points, components, border and noise: include/ecgvit_hip.h.
//
// ecgvit_tok_segments writes the dense (n, k) table once, in q order; every pair sweep reads such tables and knows nothing of the store.
// A sweep gives a workgroup 256 * R rows, R per thread in registers (row b * 256 R + r * 256 + tid), and streams the other side through LDS in
// tiles of DBSCAN_TILE segments: every lane reads the same j, so an LDS read is a broadcast.  Columns past the table are NaN in the tile: they
// fail the comparison like any non-finite segment, so the inner loop has no bound to test.  Each (row, j) decision is tok_d2(row, j) <= eps2.
//   count   rows = cols = all segments; a row's count of neighbours (itself included) stays in a register, one plain store at the end.
//   link    rows = cols = the core segments in ascending q, j < i only; an edge joins two trees of the union-find forest parent[m].
//   border  rows = the non-core segments, cols = the core segments; the smallest label among a row's core neighbours, or -1.
//
// The union-find (link).  parent[x] <= x always.  find walks down with relaxed agent-scope loads.  unite(a, b) takes the two roots, hooks the
// larger under the smaller with atomicMin, and when the value it gets back shows that the larger was no root any more (its parent `old` had
// been set by another lane), it goes on with (old, the smaller): whichever of the two atomicMin left in parent[] the larger still reaches, and
// the other is what this lane now owes.  Every value ever stored in parent[x] stays connected to x through parent[] and what running lanes
// still owe, so reading a stale value is harmless, and when the last lane is done parent[] alone connects what the edges connect.  Every loop
// strictly descends indices: each ends, and none waits for another workgroup.  The root of a tree is its smallest index, whatever the order.
#include "tok_common.h"

#define DBSCAN_TILE ECGVIT_TOK_DBSCAN_TILE               // segments per LDS tile of the column side
#define DBSCAN_ROWS(K) ((K) == 32 ? 2 : 4)               // rows per thread: 32 / 64 / 64 registers at k = 8 / 16 / 32

enum { DB_COUNT = 0, DB_LINK = 1, DB_BORDER = 2 };

__device__ __forceinline__ int db_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int db_find(const int32_t *parent, int x) {
    for (;;) {
        const int p = db_load(parent + x);
        if (p >= x) return x;                            // (p == x: a root; p > x never is stored)
        x = p;
    }
}

// -> the root both end under, as far as this lane saw it
__device__ __forceinline__ int db_unite(int32_t *parent, int a, int b) {
    for (;;) {
        a = db_find(parent, a);
        b = db_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }    // a: the larger root, hooked under b
        const int old = atomicMin(parent + a, b);
        if (old == a) return b;                          // a was a root: done
        a = old;                                         // a had been hooked meanwhile (old < a): unite what it pointed to with b
    }
}

template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_segments_kernel(TokStore st, int64_t n_seg, int C, float *__restrict__ segs, float *__restrict__ means,
                                                                    int64_t *__restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    if (p >= n_seg) return;
    const int c = blockIdx.y;
    const TokSeg g = tok_locate(st, c, p);
    float v[K];
    const float mean = tok_load<K>(st, c, g, v);
    const int64_t lo = st.seg_cum[g.r], n_r = st.seg_cum[g.r + 1] - lo;
    const int64_t q = (int64_t)C * lo + (int64_t)c * n_r + g.s;
    f32x4 *__restrict__ o = reinterpret_cast<f32x4 *>(segs + q * K);
#pragma unroll
    for (int e = 0; e < K; e += 4) {
        f32x4 w;
        w[0] = v[e]; w[1] = v[e + 1]; w[2] = v[e + 2]; w[3] = v[e + 3];
        o[e / 4] = w;
    }
    means[q] = mean;
    if (dst) dst[q] = g.dst;
}

// rows [row0, row1) of `rows` against columns [0, ncols) of `cols` (DB_LINK: rows == cols, and a row meets the columns below it only).
// aux: DB_LINK parent (read and written), DB_BORDER the columns' labels.  out: DB_COUNT the counts, DB_BORDER the labels; int32 [row index].
template <int K, int MODE>
__global__ __launch_bounds__(TOK_THREADS) void dbscan_sweep_kernel(const float *__restrict__ rows, const float *__restrict__ cols, int ncols, float eps2,
                                                                    int row0, int row1, int32_t *aux, int32_t *__restrict__ out) {
    constexpr int R = DBSCAN_ROWS(K), K4 = K / 4;
    __shared__ f32x4 tile[DBSCAN_TILE * K4];
    __shared__ int32_t taux[DBSCAN_TILE];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)row0 + (int64_t)blockIdx.x * (TOK_THREADS * R);
    float v[R][K];
    int acc[R];
    bool live[R];
    int last = -1;                                       // the block's last live row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = base + r * TOK_THREADS + tid;
        live[r] = i < row1;
#pragma unroll
        for (int e = 0; e < K; ++e) v[r][e] = 0.f;
        if (live[r]) {
            const f32x4 *__restrict__ src = reinterpret_cast<const f32x4 *>(rows + i * K);
#pragma unroll
            for (int e = 0; e < K4; ++e) {
                const f32x4 w = src[e];
                v[r][4 * e] = w[0]; v[r][4 * e + 1] = w[1]; v[r][4 * e + 2] = w[2]; v[r][4 * e + 3] = w[3];
            }
        }
        acc[r] = MODE == DB_COUNT ? 0 : MODE == DB_BORDER ? 0x7FFFFFFF : (live[r] ? db_find(aux, (int)i) : 0);
    }
    {
        const int64_t end = base + TOK_THREADS * R < row1 ? base + TOK_THREADS * R : row1;
        last = (int)(end - 1);
    }
    const int jend = MODE == DB_LINK ? (last < ncols ? last : ncols) : ncols;      // link: columns j < i <= last
    for (int j0 = 0; j0 < jend; j0 += DBSCAN_TILE) {
        __syncthreads();                                 // the previous tile has been read
#pragma unroll
        for (int t = 0; t < K4; ++t) {
            const int idx = t * TOK_THREADS + tid, j = j0 + idx / K4;
            f32x4 w;
            w[0] = w[1] = w[2] = w[3] = __builtin_nanf("");
            if (j < ncols) w = reinterpret_cast<const f32x4 *>(cols)[(int64_t)j0 * K4 + idx];
            tile[idx] = w;
        }
        if (MODE != DB_COUNT && tid < DBSCAN_TILE) {
            const int j = j0 + tid;
            taux[tid] = j < ncols ? (MODE == DB_LINK ? db_find(aux, j) : aux[j]) : 0;
        }
        __syncthreads();
#pragma unroll 2
        for (int jj = 0; jj < DBSCAN_TILE; ++jj) {
            float c[K];
#pragma unroll
            for (int e = 0; e < K4; ++e) {
                const f32x4 w = tile[jj * K4 + e];
                c[4 * e] = w[0]; c[4 * e + 1] = w[1]; c[4 * e + 2] = w[2]; c[4 * e + 3] = w[3];
            }
            const int a = MODE == DB_COUNT ? 0 : taux[jj];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool near = tok_d2<K>(v[r], c) <= eps2;
                if (MODE == DB_COUNT) {
                    acc[r] += near ? 1 : 0;
                } else if (MODE == DB_BORDER) {
                    acc[r] = near && a < acc[r] ? a : acc[r];
                } else {
                    const int64_t i = base + r * TOK_THREADS + tid;
                    if (near && live[r] && (int64_t)(j0 + jj) < i && a != acc[r]) acc[r] = db_unite(aux, acc[r], a);
                }
            }
        }
    }
    if (MODE == DB_LINK) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t i = base + r * TOK_THREADS + tid;
        if (live[r]) out[i] = MODE == DB_BORDER && acc[r] == 0x7FFFFFFF ? -1 : acc[r];
    }
}

__global__ __launch_bounds__(TOK_THREADS) void dbscan_flatten_kernel(const int32_t *parent, int m, int32_t *__restrict__ root) {
    const int64_t i = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    if (i < m) root[i] = db_find(parent, (int)i);
}

// =====================================================================================================
// entry points
// =====================================================================================================
static inline bool db_k_ok(int k) { return k == 8 || k == 16 || k == 32; }
static inline int db_rows_per_block(int k) { return TOK_THREADS * DBSCAN_ROWS(k); }

int ecgvit_tok_dbscan_tile(void) { return DBSCAN_TILE; }
int ecgvit_tok_dbscan_rows(int k) { return db_k_ok(k) ? db_rows_per_block(k) : 0; }

int ecgvit_tok_segments(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                        const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, float *segs, float *means,
                        int64_t *dst, void *stream) {
    if (!tok_store_ok(x, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, pad) || !tok_al(segs, 16) || !tok_al(means, 4) || (dst && !tok_al(dst, 8)))
        return ECGVIT_EINVAL;
    if (n_seg > 0x7FFFFFFFll / C) return ECGVIT_EINVAL;  // C * n_seg >= 2^31: past the int32 indices of the sweeps
    const int64_t blocks = (n_seg + TOK_THREADS - 1) / TOK_THREADS;
    const TokStore st = tok_store(x, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, pad);
#define TOK_LAUNCH(KK) \
    hipLaunchKernelGGL(tok_segments_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, C, segs, means, dst)
    TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

static inline bool db_sweep_ok(const float *rows, int nrows, const float *cols, int ncols, int k, float eps2, int row0, int row1) {
    return tok_al(rows, 16) && tok_al(cols, 16) && db_k_ok(k) && nrows >= 1 && ncols >= 1 && eps2 >= 0.f && eps2 < __builtin_inff() && row0 >= 0 &&
           row0 < row1 && row1 <= nrows;
}

#define DB_SWEEP(MODE, rows, cols, ncols, aux, out)                                                                                          \
    do {                                                                                                                                     \
        const int rpb__ = db_rows_per_block(k);                                                                                              \
        const unsigned blocks__ = (unsigned)(((int64_t)row1 - row0 + rpb__ - 1) / rpb__);                                                    \
        if (k == 8)                                                                                                                          \
            hipLaunchKernelGGL((dbscan_sweep_kernel<8, MODE>), dim3(blocks__), dim3(TOK_THREADS), 0, as_stream(stream), rows, cols, ncols, eps2, row0, \
                               row1, aux, out);                                                                                              \
        else if (k == 16)                                                                                                                    \
            hipLaunchKernelGGL((dbscan_sweep_kernel<16, MODE>), dim3(blocks__), dim3(TOK_THREADS), 0, as_stream(stream), rows, cols, ncols, eps2, row0, \
                               row1, aux, out);                                                                                              \
        else                                                                                                                                 \
            hipLaunchKernelGGL((dbscan_sweep_kernel<32, MODE>), dim3(blocks__), dim3(TOK_THREADS), 0, as_stream(stream), rows, cols, ncols, eps2, row0, \
                               row1, aux, out);                                                                                              \
        ECGVIT_CHECK_LAUNCH();                                                                                                               \
    } while (0)

int ecgvit_tok_dbscan_count(const float *segs, int n, int k, float eps2, int row0, int row1, int32_t *count, void *stream) {
    if (!db_sweep_ok(segs, n, segs, n, k, eps2, row0, row1) || !tok_al(count, 4)) return ECGVIT_EINVAL;
    DB_SWEEP(DB_COUNT, segs, segs, n, (int32_t *)nullptr, count);
    return ECGVIT_OK;
}

int ecgvit_tok_dbscan_link(const float *core, int m, int k, float eps2, int row0, int row1, int32_t *parent, void *stream) {
    if (!db_sweep_ok(core, m, core, m, k, eps2, row0, row1) || !tok_al(parent, 4)) return ECGVIT_EINVAL;
    DB_SWEEP(DB_LINK, core, core, m, parent, (int32_t *)nullptr);
    return ECGVIT_OK;
}

int ecgvit_tok_dbscan_flatten(const int32_t *parent, int m, int32_t *root, void *stream) {
    if (!tok_al(parent, 4) || !tok_al(root, 4) || m < 1) return ECGVIT_EINVAL;
    hipLaunchKernelGGL(dbscan_flatten_kernel, dim3((unsigned)(((int64_t)m + TOK_THREADS - 1) / TOK_THREADS)), dim3(TOK_THREADS), 0, as_stream(stream),
                       parent, m, root);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_tok_dbscan_border(const float *rows, int nrows, const float *core, const int32_t *core_label, int m, int k, float eps2, int row0, int row1,
                             int32_t *label, void *stream) {
    if (!db_sweep_ok(rows, nrows, core, m, k, eps2, row0, row1) || !tok_al(core_label, 4) || !tok_al(label, 4)) return ECGVIT_EINVAL;
    DB_SWEEP(DB_BORDER, rows, core, m, const_cast<int32_t *>(core_label), label);
    return ECGVIT_OK;
}
