// Scalable k-means++ (k-means||) seeding for the segment tokenizer (tokenizer.EcgTokenizer.kmeans_parallel): a few oversampling rounds over the
// store, then weighted k-means++ over the candidates.  Contract, the rule of every step and the layout of `info`: include/ecgvit_hip_tok_scalable.h.
// A segment has the bits every tokenizer kernel loads (tok_load), a distance is the unfused chain (tok_d2), a weight the seeding's integer
// (tok_quant): tok_common.h.  No kernel here waits for another workgroup; the row counts travel through `info` in device memory, so the whole
// seeding is enqueued without a host read.
//
// Register budgets (256-thread workgroups unless said; held by tests/test_tokenizer_scalable.py from the code objects; no spill, no scratch):
//   kmpar_fold_kernel       <= 256 VGPRs: four segments of K samples stay in registers (128 at K = 32); two workgroups per CU
//   kmpar_recluster_kernel  <= 128 VGPRs: 1024 threads are four waves per SIMD
//   every other kernel      <= 64 VGPRs: streaming passes over closest / owner, eight waves per SIMD
#include "tok_common.h"
#include "../../include/ecgvit_hip_tok_scalable.h"

#define KMPAR_SPAN ECGVIT_TOK_SEED_SPAN                    // segments per workgroup of the fold: four per thread
#define KMPAR_PER (KMPAR_SPAN / TOK_THREADS)
#define KMPAR_ROWS ECGVIT_TOK_SCALABLE_FOLD_ROWS           // table rows per LDS chunk (32 KiB at K = 32)
#define KMPAR_SEL ECGVIT_TOK_SCALABLE_SELECT_SPAN          // segments per workgroup of the selection: one per thread
#define KMPAR_TMAX ECGVIT_TOK_MAX_LOCAL_TRIALS
#define KMPAR_WIDE 1024                                    // threads of the one-workgroup kernels (potential, scan, recluster)
#define KMPAR_HEAD ECGVIT_TOK_SCALABLE_INFO_HEAD
// info: [0] n_c, rows of the table; [1] rows folded so far; [2] the row the current round appends from; [3] rows it appends
#define KMPAR_NC 0
#define KMPAR_FOLDED 1
#define KMPAR_BASE 2
#define KMPAR_APP 3
static_assert(KMPAR_SEL == TOK_THREADS && KMPAR_SPAN % TOK_THREADS == 0, "one segment per thread of the selection, whole segments per thread of the fold");

// row 0 of the table: segment `first`
template <int K>
__global__ __launch_bounds__(WAVE) void kmpar_init_kernel(TokStore st, int64_t n_seg, int64_t first, float *__restrict__ table,
                                                          int64_t *__restrict__ cand_g, u64 *__restrict__ info) {
    if (threadIdx.x) return;
    const int c = (int)(first / n_seg);
    const TokSeg g = tok_locate(st, c, first % n_seg);
    float v[K];
    tok_load<K>(st, c, g, v);
#pragma unroll
    for (int e = 0; e < K; ++e) table[e] = v[e];
    cand_g[0] = first;
    info[KMPAR_NC] = 1;
}

// =====================================================================================================
// fold: rows [info[1], info[0]) of the table against every segment.  The rows of a chunk are read from LDS at one address per instruction (a
// broadcast); a thread's four segments take them in row order with a strict <.  fresh: closest and owner have never been written.
// =====================================================================================================
template <int K>
__global__ __launch_bounds__(TOK_THREADS) void kmpar_fold_kernel(TokStore st, int64_t n_seg, int fresh, const u64 *__restrict__ info,
                                                                  const float *__restrict__ table, float *__restrict__ closest,
                                                                  int32_t *__restrict__ owner, u64 *__restrict__ block_sums,
                                                                  const uint32_t *__restrict__ amax, int fbase) {
    __shared__ __attribute__((aligned(16))) float rows[KMPAR_ROWS * K];
    __shared__ u64 red[TOK_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y;
    const int lo = (int)info[KMPAR_FOLDED], hi = (int)info[KMPAR_NC];
    float v[KMPAR_PER][K], cl[KMPAR_PER];
    int ow[KMPAR_PER];
    bool live[KMPAR_PER];
#pragma unroll
    for (int j = 0; j < KMPAR_PER; ++j) {
        const int64_t p = (int64_t)blockIdx.x * KMPAR_SPAN + j * TOK_THREADS + tid;
        live[j] = p < n_seg;
        cl[j] = __builtin_inff();
        ow[j] = -1;
#pragma unroll
        for (int e = 0; e < K; ++e) v[j][e] = 0.f;
        if (live[j]) {
            const TokSeg g = tok_locate(st, c, p);
            tok_load<K>(st, c, g, v[j]);
            if (!fresh) {
                cl[j] = closest[(int64_t)c * n_seg + p];
                ow[j] = owner[(int64_t)c * n_seg + p];
            }
        }
    }
    for (int r0 = lo; r0 < hi; r0 += KMPAR_ROWS) {
        const int n = hi - r0 < KMPAR_ROWS ? hi - r0 : KMPAR_ROWS;
        __syncthreads();   // the previous chunk has been read
        for (int i = tid; i < n * K; i += TOK_THREADS) rows[i] = table[(int64_t)r0 * K + i];
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < n; ++r) {
#pragma unroll
            for (int j = 0; j < KMPAR_PER; ++j) {
                const float d = tok_d2<K>(v[j], rows + r * K);
                const bool lt = d < cl[j];               // (a NaN distance leaves what is there)
                cl[j] = lt ? d : cl[j];
                ow[j] = lt ? r0 + r : ow[j];
            }
        }
    }
    const int F = tok_seed_f(fbase, *amax);
    u64 a = 0;
#pragma unroll
    for (int j = 0; j < KMPAR_PER; ++j) {
        const int64_t p = (int64_t)blockIdx.x * KMPAR_SPAN + j * TOK_THREADS + tid;
        if (live[j]) {
            if (fresh || hi > lo) {
                closest[(int64_t)c * n_seg + p] = cl[j];
                owner[(int64_t)c * n_seg + p] = ow[j];
            }
            a += tok_quant(cl[j], F);
        }
    }
    a = wave_sum_u64(a);
    if (lane == 0) red[wave] = a;
    __syncthreads();
    if (tid == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < TOK_THREADS / WAVE; ++w) s += red[w];
        block_sums[(int64_t)c * gridDim.x + blockIdx.x] = s;
    }
}

// the potential: the sum of the fold's partials -> info[slot]; every row of the table is folded now
__global__ __launch_bounds__(KMPAR_WIDE) void kmpar_pot_kernel(const u64 *__restrict__ block_sums, int64_t NB, u64 *__restrict__ info, int slot) {
    __shared__ u64 wsum[KMPAR_WIDE / WAVE];
    const int tid = threadIdx.x;
    u64 a = 0;
    for (int64_t i = tid; i < NB; i += KMPAR_WIDE) a += block_sums[i];
    a = wave_sum_u64(a);
    if ((tid & 63) == 0) wsum[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < KMPAR_WIDE / WAVE; ++w) s += wsum[w];
        info[slot] = s;
        info[KMPAR_FOLDED] = info[KMPAR_NC];
    }
}

// =====================================================================================================
// select: a pure function of (key, g, closest(g), pot), evaluated twice -- once to count, once to scatter
// =====================================================================================================
__device__ __forceinline__ u64 kmpar_mix(u64 key, u64 g) {
    u64 z = key + g * 0x9E3779B97F4A7C15ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// q > 0 and ((u pot) >> 53) < ell q: the left side is below 2^63, the right side a 128-bit product
__device__ __forceinline__ bool kmpar_take(u64 key, u64 g, float cl, int F, u64 pot, u64 ell) {
    const u64 q = tok_quant(cl, F);
    if (q == 0) return false;
    const u64 lhs = tok_target(kmpar_mix(key, g) >> 11, pot);
    return __umul64hi(ell, q) != 0 || lhs < ell * q;
}

__global__ __launch_bounds__(TOK_THREADS) void kmpar_select_count_kernel(int64_t n_seg, const float *__restrict__ closest, u64 key, u64 ell,
                                                                          const u64 *__restrict__ info, int pot_slot, uint32_t *__restrict__ counts,
                                                                          const uint32_t *__restrict__ amax, int fbase) {
    __shared__ uint32_t wcnt[TOK_THREADS / WAVE];
    const int tid = threadIdx.x, c = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * KMPAR_SEL + tid;
    const u64 g = (u64)c * (u64)n_seg + (u64)p;
    const bool take = p < n_seg && kmpar_take(key, g, closest[g], tok_seed_f(fbase, *amax), info[pot_slot], ell);
    const uint32_t n = (uint32_t)__popcll(__ballot(take));
    if ((tid & 63) == 0) wcnt[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < TOK_THREADS / WAVE; ++w) s += wcnt[w];
        counts[(int64_t)c * gridDim.x + blockIdx.x] = s;
    }
}

// counts -> exclusive offsets in place, in workgroup order (= ascending g); the round's bookkeeping
__global__ __launch_bounds__(KMPAR_WIDE) void kmpar_select_scan_kernel(uint32_t *__restrict__ counts, int64_t NB, u64 *__restrict__ info, int round,
                                                                        int n_rounds, u64 cap) {
    __shared__ u64 wsum[KMPAR_WIDE / WAVE];
    __shared__ u64 s_total;
    const int tid = threadIdx.x;
    const int64_t chunk = (NB + KMPAR_WIDE - 1) / KMPAR_WIDE;
    const int64_t lo = tid * chunk < NB ? tid * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    u64 cs = 0;
    for (int64_t i = lo; i < hi; ++i) cs += counts[i];
    const u64 incl = block_scan_u64(cs, wsum);
    u64 run = incl - cs;
    for (int64_t i = lo; i < hi; ++i) {
        const uint32_t n = counts[i];
        counts[i] = (uint32_t)run;                       // (fewer than 2^32 segments in all)
        run += n;
    }
    if (tid == KMPAR_WIDE - 1) s_total = incl;
    __syncthreads();
    if (tid == 0) {
        const u64 total = s_total, app = total < cap ? total : cap;
        info[KMPAR_BASE] = info[KMPAR_NC];
        info[KMPAR_APP] = app;
        info[KMPAR_NC] += app;
        info[KMPAR_HEAD + round] = total;
        info[KMPAR_HEAD + n_rounds + round] = total - app;
    }
}

template <int K>
__global__ __launch_bounds__(TOK_THREADS) void kmpar_select_scatter_kernel(TokStore st, int64_t n_seg, const float *__restrict__ closest, u64 key, u64 ell,
                                                                            const u64 *__restrict__ info, int pot_slot,
                                                                            const uint32_t *__restrict__ offsets, float *__restrict__ table,
                                                                            int64_t *__restrict__ cand_g, const uint32_t *__restrict__ amax, int fbase) {
    __shared__ uint32_t wcnt[TOK_THREADS / WAVE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * KMPAR_SEL + tid;
    const u64 g = (u64)c * (u64)n_seg + (u64)p;
    const bool take = p < n_seg && kmpar_take(key, g, closest[g], tok_seed_f(fbase, *amax), info[pot_slot], ell);
    const u64 mask = __ballot(take);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    u64 pos = (u64)offsets[(int64_t)c * gridDim.x + blockIdx.x] + (u64)__popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += wcnt[w];
    if (take && pos < info[KMPAR_APP]) {                 // the round's first `cap` in ascending g; the rest is dropped
        const int64_t row = (int64_t)(info[KMPAR_BASE] + pos);
        const TokSeg sg = tok_locate(st, c, p);
        float v[K];
        tok_load<K>(st, c, sg, v);
#pragma unroll
        for (int e = 0; e < K; ++e) table[row * K + e] = v[e];
        cand_g[row] = (int64_t)g;
    }
}

// =====================================================================================================
// weights: w[owner(g)] += 1 over the segments that have an owner (closest finite).  The lanes of a wave that name one row are counted by a
// ballot and added by one of them: consecutive segments share owners, and same-address atomics are what this pass would otherwise wait for.
// =====================================================================================================
__global__ __launch_bounds__(TOK_THREADS) void kmpar_weights_kernel(int64_t total, const int32_t *__restrict__ owner, u64 *__restrict__ weights) {
    const int64_t g = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int o = g < total ? owner[g] : -1;
    bool todo = o >= 0;
    for (u64 m = __ballot(todo); m; m = __ballot(todo)) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int lo = __shfl(o, leader, 64);
        const bool same = todo && o == lo;
        const u64 sm = __ballot(same);
        if (lane == leader) atomicAdd(weights + o, (u64)__popcll(sm));
        todo = todo && !same;
    }
}

// =====================================================================================================
// recluster: weighted greedy k-means++ over the n_c rows of the table, one workgroup, all V centres in one launch.  rc[j] = the distance of
// row j to the nearest chosen row.  Per centre: pass A applies the row chosen last to rc and sums w q(rc) over a thread's CONTIGUOUS chunk of
// rows (a scan over the threads finds each target's chunk, one thread walks it); pass B weighs every row under each of the T candidates in turn
// (rows strided over the threads: integer sums have no order).
// =====================================================================================================
template <int K>
__global__ __launch_bounds__(KMPAR_WIDE) void kmpar_recluster_kernel(const u64 *__restrict__ info, const float *__restrict__ table,
                                                                      const int64_t *__restrict__ cand_g, const u64 *__restrict__ weights, float *rc,
                                                                      int V, int T, u64 u0, const u64 *__restrict__ u53, float *__restrict__ centers,
                                                                      int64_t *__restrict__ indices, const uint32_t *__restrict__ amax, int fbase) {
    __shared__ u64 wsum[KMPAR_WIDE / WAVE], red[KMPAR_WIDE / WAVE][KMPAR_TMAX], tgt[KMPAR_TMAX];
    __shared__ u64 s_total;
    __shared__ int cj[KMPAR_TMAX], s_win;
    __shared__ float crow[(KMPAR_TMAX + 1) * K];         // row 0: the row chosen last; rows 1 .. T: the candidates
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = (int)info[KMPAR_NC];
    if (n < V) return;                                   // too few candidates: the caller reads info[0] and refuses
    const int F = tok_seed_f(fbase, *amax);
    const int chunk = (n + KMPAR_WIDE - 1) / KMPAR_WIDE;
    const int lo = tid * chunk < n ? tid * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    // centre 0: the smallest j whose running sum of w exceeds (u0 sum w) >> 53
    {
        u64 cs = 0;
        for (int j = lo; j < hi; ++j) cs += weights[j];
        const u64 incl = block_scan_u64(cs, wsum), excl = incl - cs;
        if (tid == KMPAR_WIDE - 1) s_total = incl;
        if (tid == 0) cj[0] = 0;
        __syncthreads();
        const u64 tg = tok_target(u0, s_total);
        if (s_total && tg >= excl && tg < incl) {
            u64 run = excl;
            for (int j = lo; j < hi; ++j) {
                const u64 b = weights[j];
                if (tg < run + b) { cj[0] = j; break; }
                run += b;
            }
        }
        __syncthreads();
        if (tid < K) {
            const float w = table[(int64_t)cj[0] * K + tid];
            crow[tid] = w;
            centers[tid] = w;
        }
        if (tid == 0) indices[0] = cand_g[cj[0]];
        __syncthreads();
    }
    for (int s = 1; s < V; ++s) {
        // pass A: the row chosen last, the weights the step draws from, their scan
        u64 cs = 0;
        for (int j = lo; j < hi; ++j) {
            float v[K];
#pragma unroll
            for (int e = 0; e < K; ++e) v[e] = table[(int64_t)j * K + e];
            const float d = tok_d2<K>(v, crow);
            float r = s == 1 ? __builtin_inff() : rc[j];
            r = d < r ? d : r;
            rc[j] = r;
            cs += weights[j] * tok_quant(r, F);
        }
        const u64 incl = block_scan_u64(cs, wsum), excl = incl - cs;
        if (tid == KMPAR_WIDE - 1) s_total = incl;
        if (tid < T) cj[tid] = 0;                        // pot == 0: row 0, what searchsorted returns there
        __syncthreads();
        const u64 pot = s_total;
        if (tid < T) tgt[tid] = tok_target(u53[(int64_t)(s - 1) * T + tid], pot);
        __syncthreads();                                 // (also: every rc[j] of pass A is visible to the workgroup)
        if (pot) {
            for (int t = 0; t < T; ++t) {
                const u64 tg = tgt[t];
                if (tg >= excl && tg < incl) {           // one thread: the chunks partition [0, pot) and tg < pot
                    u64 run = excl;
                    for (int j = lo; j < hi; ++j) {
                        const u64 b = weights[j] * tok_quant(rc[j], F);
                        if (tg < run + b) { cj[t] = j; break; }
                        run += b;
                    }
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < T * K; i += KMPAR_WIDE) crow[K + i] = table[(int64_t)cj[i / K] * K + i % K];
        __syncthreads();
        // pass B: the potential each candidate leaves
#pragma unroll 1
        for (int t = 0; t < T; ++t) {                    // one candidate at a time: its row and one accumulator in registers (the table is cache-resident)
            float cr[K];
#pragma unroll
            for (int e = 0; e < K; ++e) cr[e] = crow[(t + 1) * K + e];
            u64 a = 0;
            for (int j = tid; j < n; j += KMPAR_WIDE) {
                float v[K];
#pragma unroll
                for (int e = 0; e < K; ++e) v[e] = table[(int64_t)j * K + e];
                const float r = rc[j];
                const float d = tok_d2<K>(v, cr);
                a += weights[j] * tok_quant(d < r ? d : r, F);
            }
            a = wave_sum_u64(a);
            if (lane == 0) red[wave][t] = a;
        }
        __syncthreads();
        if (tid == 0) {                                  // the smallest potential; equal potentials go to the smaller trial
            u64 best = 0;
            int win = 0;
            for (int t = 0; t < T; ++t) {
                u64 x = 0;
                for (int w = 0; w < KMPAR_WIDE / WAVE; ++w) x += red[w][t];
                if (t == 0 || x < best) { best = x; win = t; }
            }
            s_win = win;
            indices[s] = cand_g[cj[win]];
        }
        __syncthreads();
        float w = 0.f;
        if (tid < K) w = crow[(s_win + 1) * K + tid];
        __syncthreads();
        if (tid < K) {
            crow[tid] = w;
            centers[(int64_t)s * K + tid] = w;
        }
        __syncthreads();
    }
}

// =====================================================================================================
// entry points
// =====================================================================================================
static inline bool kmpar_shape_ok(int C, int64_t n_seg, int V, int k, int n_trials, int n_rounds, int64_t cap) {
    return V >= 1 && V <= ECGVIT_TOK_MAX_CLUSTERS && (k == 8 || k == 16 || k == 32) && C >= 1 && C <= 65535 && n_seg >= 1 && n_trials >= 1 &&
           n_trials <= KMPAR_TMAX && n_rounds >= 1 && n_rounds <= ECGVIT_TOK_SCALABLE_MAX_ROUNDS && cap >= 1 && cap <= ECGVIT_TOK_MAX_CLUSTERS &&
           1 + (int64_t)n_rounds * cap <= ECGVIT_TOK_MAX_CLUSTERS && n_seg <= 0xFFFFFFFFll / C && (int64_t)V <= (int64_t)C * n_seg;
}

struct KmparLayout {
    int64_t rows, table, rc, sums, counts, closest, owner, bytes, NB, NS;
};

static inline int64_t kmpar_up(int64_t b) { return (b + 15) & ~15ll; }

static KmparLayout kmpar_layout(int C, int64_t n_seg, int k, int n_rounds, int64_t cap) {
    KmparLayout l;
    l.rows = 1 + (int64_t)n_rounds * cap;
    l.NB = (n_seg + KMPAR_SPAN - 1) / KMPAR_SPAN * C;
    l.NS = (n_seg + KMPAR_SEL - 1) / KMPAR_SEL * C;
    l.table = 16;                                        // the maximum's bits at 0
    l.rc = l.table + kmpar_up(l.rows * k * 4);
    l.sums = l.rc + kmpar_up(l.rows * 4);
    l.counts = l.sums + kmpar_up(l.NB * 8);
    l.closest = l.counts + kmpar_up(l.NS * 4);
    l.owner = l.closest + kmpar_up((int64_t)C * n_seg * 4);
    l.bytes = l.owner + kmpar_up((int64_t)C * n_seg * 4);
    return l;
}

int64_t ecgvit_tok_scalable_workspace(int C, int64_t n_seg, int V, int k, int n_trials, int n_rounds, int64_t cap) {
    if (!kmpar_shape_ok(C, n_seg, V, k, n_trials, n_rounds, cap)) return 0;
    return kmpar_layout(C, n_seg, k, n_rounds, cap).bytes;
}

int ecgvit_tok_scalable_seed(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                             const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, int V, int n_trials,
                             int n_rounds, int64_t ell, int64_t cap, int64_t first, const uint64_t *keys, uint64_t u0, const uint64_t *u53,
                             float *centers, int64_t *indices, int64_t *cand_g, uint64_t *weights, uint64_t *info, void *workspace,
                             int keep_amax, void *stream) {
    if (!tok_store_ok(x, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, pad) || !kmpar_shape_ok(C, n_seg, V, k, n_trials, n_rounds, cap) ||
        ell < 1 || ell > ECGVIT_TOK_MAX_CLUSTERS || first < 0 || first >= (int64_t)C * n_seg || !keys || u0 >> 53 || (V > 1 && !tok_al(u53, 8)) ||
        !tok_al(centers, 4) || !tok_al(indices, 8) || !tok_al(cand_g, 8) || !tok_al(weights, 8) || !tok_al(info, 8) || !tok_al(workspace, 16) ||
        (keep_amax != 0 && keep_amax != 1))
        return ECGVIT_EINVAL;
    const KmparLayout l = kmpar_layout(C, n_seg, k, n_rounds, cap);
    const int64_t B = l.NB / C, BS = l.NS / C, total = (int64_t)C * n_seg, wblocks = (total + TOK_THREADS - 1) / TOK_THREADS;
    if (B > 0x7FFFFFFFll || BS > 0x7FFFFFFFll || wblocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
    hipStream_t s = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    uint32_t *amax = reinterpret_cast<uint32_t *>(ws);
    float *table = reinterpret_cast<float *>(ws + l.table), *rc = reinterpret_cast<float *>(ws + l.rc);
    u64 *block_sums = reinterpret_cast<u64 *>(ws + l.sums), *inf = reinterpret_cast<u64 *>(info), *w = reinterpret_cast<u64 *>(weights);
    uint32_t *counts = reinterpret_cast<uint32_t *>(ws + l.counts);
    float *closest = reinterpret_cast<float *>(ws + l.closest);
    int32_t *owner = reinterpret_cast<int32_t *>(ws + l.owner);
    const int fbase = tok_seed_fbase(C, n_seg, k), slot0 = KMPAR_HEAD + 2 * n_rounds;
    const TokStore st = tok_store(x, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, pad);
    if (hipMemsetAsync(info, 0, (size_t)(KMPAR_HEAD + 3 * n_rounds + 1) * 8, s) != hipSuccess ||
        hipMemsetAsync(weights, 0, (size_t)l.rows * 8, s) != hipSuccess)
        return ECGVIT_ELAUNCH;
    if (!keep_amax) {
        if (hipMemsetAsync(amax, 0, 16, s) != hipSuccess) return ECGVIT_ELAUNCH;
        const int rc_ = tok_launch_amax(st, C, n_seg, k, amax, s);
        if (rc_ != ECGVIT_OK) return rc_;
    }
#define KMPAR_INIT(KK) hipLaunchKernelGGL(kmpar_init_kernel<KK>, dim3(1), dim3(WAVE), 0, s, st, n_seg, first, table, cand_g, inf)
    TOK_BY_K(k, KMPAR_INIT);
#undef KMPAR_INIT
    ECGVIT_CHECK_LAUNCH();
    for (int r = 0; r <= n_rounds; ++r) {                // round n_rounds: the last fold, the weights, the recluster
        const int fresh = r == 0;
#define KMPAR_FOLD(KK)                                                                                                                      \
    hipLaunchKernelGGL(kmpar_fold_kernel<KK>, dim3((unsigned)B, C), dim3(TOK_THREADS), 0, s, st, n_seg, fresh, inf, table, closest, owner, \
                       block_sums, amax, fbase)
        TOK_BY_K(k, KMPAR_FOLD);
#undef KMPAR_FOLD
        ECGVIT_CHECK_LAUNCH();
        hipLaunchKernelGGL(kmpar_pot_kernel, dim3(1), dim3(KMPAR_WIDE), 0, s, block_sums, l.NB, inf, slot0 + r);
        ECGVIT_CHECK_LAUNCH();
        if (r == n_rounds) break;
        hipLaunchKernelGGL(kmpar_select_count_kernel, dim3((unsigned)BS, C), dim3(TOK_THREADS), 0, s, n_seg, closest, (u64)keys[r], (u64)ell, inf,
                           slot0 + r, counts, amax, fbase);
        ECGVIT_CHECK_LAUNCH();
        hipLaunchKernelGGL(kmpar_select_scan_kernel, dim3(1), dim3(KMPAR_WIDE), 0, s, counts, l.NS, inf, r, n_rounds, (u64)cap);
        ECGVIT_CHECK_LAUNCH();
#define KMPAR_SCATTER(KK)                                                                                                                     \
    hipLaunchKernelGGL(kmpar_select_scatter_kernel<KK>, dim3((unsigned)BS, C), dim3(TOK_THREADS), 0, s, st, n_seg, closest, (u64)keys[r], (u64)ell, \
                       inf, slot0 + r, counts, table, cand_g, amax, fbase)
        TOK_BY_K(k, KMPAR_SCATTER);
#undef KMPAR_SCATTER
        ECGVIT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(kmpar_weights_kernel, dim3((unsigned)wblocks), dim3(TOK_THREADS), 0, s, total, owner, w);
    ECGVIT_CHECK_LAUNCH();
#define KMPAR_RECLUSTER(KK)                                                                                                                \
    hipLaunchKernelGGL(kmpar_recluster_kernel<KK>, dim3(1), dim3(KMPAR_WIDE), 0, s, inf, table, cand_g, w, rc, V, n_trials, (u64)u0,           \
                       reinterpret_cast<const u64 *>(u53), centers, indices, amax, fbase)
    TOK_BY_K(k, KMPAR_RECLUSTER);
#undef KMPAR_RECLUSTER
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
