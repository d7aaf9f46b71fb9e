// The segment tokenizer (tokenizer.EcgTokenizer; the reference's models/ecg_tokenizer.py): nearest-centre assignment, the Lloyd update, the
// k-means++ seeding and the decode, over a record store addressed as fit_stats.hip addresses it.  Contract, padding rule and the order of every sum: include/ecgvit_hip.h.
//
// Work is laid out per lead: workgroup (b, c) takes positions [b * span, (b + 1) * span) of lead c's segments, a position finds its record by
// a binary search in seg_cum.  The padding is applied in the segment load; no padded copy of the store exists.
#include "tok_common.h"

#define TOK_NS 4                                        // groups of 32 segments per wave: four independent accumulators
#define TOK_SPAN (TOK_THREADS / WAVE * TOK_NS * 32)     // segments per workgroup of the assign kernel (512)
#define TOK_CHUNK 8192                                  // centre floats per LDS chunk: 32 KiB, + the norms; the table is streamed chunk by chunk

// =====================================================================================================
// assign.  D = A . B + C on v_mfma_f32_32x32x2_f32 with A = 32 centres (row i on lane i & 31, sample 2 kk + (lane >> 5)), B = 32 segments
// times -2 (column j on lane j & 31, the same sample) and C = |c_i|^2 in every column: after K / 2 instructions register g of lane (j, h) is
// the score of centre (g & 3) + 8 (g >> 2) + 4 h of the tile for segment j -- the segment's operand and its 16 scores sit on the same lane,
// so the running (best score, best index) pair is two registers per segment group and never leaves the lane until the two halves meet at the
// end.  Centres are visited in ascending order with a strict <: equal scores keep the smaller index.
// LDS: the chunk of the table transposed, ct[sample][centre] (consecutive lanes read consecutive words), and its norms; rows past V are zero
// with norm +inf: never below a finite score.
// =====================================================================================================
template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_assign_kernel(TokStore st, int64_t n_seg, const float *__restrict__ centers, int V,
                                                                  const int32_t *prev_ids, int32_t *ids, float *__restrict__ means,
                                                                  float *__restrict__ dist, u64 *__restrict__ changed) {
    constexpr int KH = K / 2, VT = TOK_CHUNK / K;
    __shared__ __attribute__((aligned(16))) float ct[K * VT];
    __shared__ __attribute__((aligned(16))) float cn[VT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5, c = blockIdx.y;
    const uint32_t hmask = 0u - (uint32_t)h;
    float b[TOK_NS][KH], mean[TOK_NS], best[TOK_NS];
    int bi[TOK_NS];
    int64_t dst[TOK_NS];
    bool live[TOK_NS];
#pragma unroll
    for (int q = 0; q < TOK_NS; ++q) {
        const int64_t p = (int64_t)blockIdx.x * TOK_SPAN + (wave * TOK_NS + q) * 32 + j;
        live[q] = p < n_seg;
        best[q] = __builtin_inff();
        bi[q] = 0;
        mean[q] = 0.f;
        dst[q] = 0;
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) b[q][kk] = 0.f;
        if (live[q]) {
            const TokSeg g = tok_locate(st, c, p);
            float v[K];
            mean[q] = tok_load<K>(st, c, g, v);
            dst[q] = g.dst;
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) {   // the lane half's sample of the pair, picked on the bits: both stay in registers
                const uint32_t even = __float_as_uint(v[2 * kk]), odd = __float_as_uint(v[2 * kk + 1]);
                b[q][kk] = -2.0f * __uint_as_float((odd & hmask) | (even & ~hmask));
            }
        }
    }
    for (int v0 = 0; v0 < V; v0 += VT) {
        __syncthreads();   // the previous chunk has been read
        for (int t = tid; t < VT; t += TOK_THREADS) {
            const int row = v0 + t;
            float n2 = __builtin_inff();
            if (row < V) {
                n2 = 0.f;
#pragma unroll
                for (int e = 0; e < K; ++e) {
                    const float w = centers[(int64_t)row * K + e];
                    ct[e * VT + t] = w;
                    n2 = fmaf(w, w, n2);
                }
            } else {
#pragma unroll
                for (int e = 0; e < K; ++e) ct[e * VT + t] = 0.f;
            }
            cn[t] = n2;
        }
        __syncthreads();
        const int rows = V - v0 < VT ? V - v0 : VT;
        for (int t0 = 0; t0 < rows; t0 += 32) {
            f32x16 cinit;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 n4 = *reinterpret_cast<const f32x4 *>(&cn[t0 + 8 * g + 4 * h]);
                cinit[4 * g] = n4[0]; cinit[4 * g + 1] = n4[1]; cinit[4 * g + 2] = n4[2]; cinit[4 * g + 3] = n4[3];
            }
            f32x16 acc[TOK_NS];
#pragma unroll
            for (int q = 0; q < TOK_NS; ++q) acc[q] = cinit;
#pragma unroll
            for (int kk = 0; kk < KH; ++kk) {
                const float a = ct[(2 * kk + h) * VT + t0 + j];
#pragma unroll
                for (int q = 0; q < TOK_NS; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[q][kk], acc[q], 0, 0, 0);
            }
            const int i0 = v0 + t0 + 4 * h;
#pragma unroll
            for (int q = 0; q < TOK_NS; ++q) {
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const float s = acc[q][g];
                    const bool lt = s < best[q];
                    best[q] = lt ? s : best[q];
                    bi[q] = lt ? i0 + (g & 3) + 8 * (g >> 2) : bi[q];
                }
            }
        }
    }
    u64 nchanged = 0;
#pragma unroll
    for (int q = 0; q < TOK_NS; ++q) {
        const float ob = __shfl_xor(best[q], 32, 64);
        const int oi = __shfl_xor(bi[q], 32, 64);
        if (ob < best[q] || (ob == best[q] && oi < bi[q])) { best[q] = ob; bi[q] = oi; }
        const int id = bi[q];   // < V: index 0 unless a finite score was seen
        float part = 0.f;
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) {
            const float d = -0.5f * b[q][kk] - centers[(int64_t)id * K + 2 * kk + h];
            part = fmaf(d, d, part);
        }
        const float d2 = part + __shfl_xor(part, 32, 64);
        const bool wr = live[q] && h == 0;
        bool ch = false;
        if (wr) {
            if (prev_ids) ch = prev_ids[dst[q]] != id;
            ids[dst[q]] = id;
            means[dst[q]] = mean[q];
            if (dist) dist[dst[q]] = d2;
        }
        nchanged += (u64)__popcll(__ballot(ch));
    }
    if (changed && lane == 0 && nchanged) atomicAdd(changed, nchanged);
}

// =====================================================================================================
// update: one thread per segment.  Pass one: the absolute maximum of the mean-removed samples (non-negative floats order as integers).  Pass two:
// every sample as a fixed-point integer at the scale the maximum sets, added to its centre's int64 sum.  Pass three: the division.
// =====================================================================================================
template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_amax_kernel(TokStore st, int64_t n_seg, uint32_t *__restrict__ amax) {
    const int64_t p = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    float m = 0.f;
    if (p < n_seg) {
        const TokSeg g = tok_locate(st, blockIdx.y, p);
        float v[K];
        tok_load<K>(st, blockIdx.y, g, v);
#pragma unroll
        for (int e = 0; e < K; ++e) m = fmaxf(m, fabsf(v[e]));   // (fmaxf drops a NaN sample)
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(amax, __float_as_uint(m));
}

int tok_launch_amax(const TokStore &st, int C, int64_t n_seg, int k, uint32_t *amax, hipStream_t stream) {
    const int64_t blocks = (n_seg + TOK_THREADS - 1) / TOK_THREADS;
    if (blocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
#define TOK_LAUNCH(KK) hipLaunchKernelGGL(tok_amax_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, stream, st, n_seg, amax)
    TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_accum_kernel(TokStore st, int64_t n_seg, const int32_t *__restrict__ ids, int V,
                                                                 const uint32_t *__restrict__ amax, u64 *__restrict__ sums, u64 *__restrict__ counts) {
    const int64_t p = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    if (p >= n_seg) return;
    const TokSeg g = tok_locate(st, blockIdx.y, p);
    const int id = ids[g.dst];
    if (id < 0 || id >= V) return;
    float v[K];
    tok_load<K>(st, blockIdx.y, g, v);
    const double scale = ldexp(1.0, tok_shift(*amax));
    atomicAdd(counts + id, (u64)1);
#pragma unroll
    for (int e = 0; e < K; ++e) {
        const long long q = __double2ll_rn((double)v[e] * scale);
        if (q) atomicAdd(sums + (int64_t)id * K + e, (u64)q);   // two's complement: the unsigned sum is the signed one
    }
}

__global__ __launch_bounds__(TOK_THREADS) void tok_finish_kernel(const u64 *__restrict__ sums, const u64 *__restrict__ counts,
                                                                  const uint32_t *__restrict__ amax, int V, int K, float *__restrict__ centers,
                                                                  int64_t *__restrict__ lens) {
    const int t = blockIdx.x * TOK_THREADS + threadIdx.x;
    if (t >= V * K) return;
    const int jrow = t / K;
    const u64 n = counts[jrow];
    if (t % K == 0) lens[jrow] = (int64_t)n;
    if (n) centers[t] = (float)(ldexp((double)(long long)sums[t], -tok_shift(*amax)) / (double)n);
}

// =====================================================================================================
// k-means++ seeding (sklearn's greedy _kmeans_plusplus, every sum an integer; the contract: include/ecgvit_hip.h).  Two launches per centre:
//   sweep s  reads every segment once: applies centre s - 1 to closest[g] (a flat f32 array over g = c * n_seg + p), then weighs the segment
//            under each of the step's candidates, q_t = quant(min(closest, d2_t)), and leaves ONE u64 per (candidate, workgroup) in
//            block_sums[t][c * blocks + b] -- workgroups ascend with g; no atomics, integer addition has no order.
//   pick s   (one workgroup) sums each candidate's row to its potential, accepts the argmin as centre s, then draws the next step's candidates:
//            a chunked scan of the winner's row finds each target's workgroup, the weights of that one span are recomputed by the sweep's own
//            expression and scanned to the segment.
// Step 0 is the same pipeline with one candidate, the given first segment, from closest = +inf (which is never quantised, nor stored: the
// array is first written by sweep 1 and first read by pick 1).
// =====================================================================================================
#define SEED_SPAN ECGVIT_TOK_SEED_SPAN                    // segments per workgroup of the sweep: four per thread
#define SEED_PER (SEED_SPAN / TOK_THREADS)
#define SEED_TMAX ECGVIT_TOK_MAX_LOCAL_TRIALS             // candidates per step
#define SEED_PICK_THREADS SEED_SPAN                      // the pick scans a sweep span with one segment per thread
#define SEED_WS_CAND_G 16                                // workspace: the maximum's bits at 0, the candidates' g (int64 [16]),
#define SEED_WS_CAND_C (SEED_WS_CAND_G + SEED_TMAX * 8)  //   the candidates' segments (f32 [16][32]),
#define SEED_WS_SUMS (SEED_WS_CAND_C + SEED_TMAX * 32 * 4)   // block_sums (u64 [T][C * blocks]), then closest (f32 [C * n_seg])

template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_seed_sweep_kernel(TokStore st, int64_t n_seg, int step, int T, int64_t first,
                                                                      const float *__restrict__ centers, float *__restrict__ cand_c,
                                                                      int64_t *__restrict__ cand_g, float *__restrict__ closest,
                                                                      u64 *__restrict__ block_sums, int64_t NB, const uint32_t *__restrict__ amax,
                                                                      int fbase) {
    __shared__ float cc[(SEED_TMAX + 1) * K];            // row 0: the centre accepted by the previous pick; rows 1 .. T: the candidates
    __shared__ u64 red[TOK_THREADS / WAVE][SEED_TMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = blockIdx.y;
    if (step == 0) {                                     // the one candidate is the given segment; workgroup (0, 0) also leaves it for the pick
        if (tid == 0) {
            const int fc = (int)(first / n_seg);
            const TokSeg g = tok_locate(st, fc, first % n_seg);
            float v[K];
            tok_load<K>(st, fc, g, v);
#pragma unroll
            for (int e = 0; e < K; ++e) cc[K + e] = v[e];
            if (blockIdx.x == 0 && c == 0) {
#pragma unroll
                for (int e = 0; e < K; ++e) cand_c[e] = v[e];
                cand_g[0] = first;
            }
        }
    } else {
        for (int i = tid; i < (T + 1) * K; i += TOK_THREADS) cc[i] = i < K ? centers[(int64_t)(step - 1) * K + i] : cand_c[i - K];
    }
    __syncthreads();
    const int F = tok_seed_f(fbase, *amax);
    // the span's four segments per thread stay in registers; the centre of the previous pick is applied once, then each candidate is one pass
    float v[SEED_PER][K], cl[SEED_PER];
    bool live[SEED_PER];
#pragma unroll
    for (int j = 0; j < SEED_PER; ++j) {
        const int64_t p = (int64_t)blockIdx.x * SEED_SPAN + j * TOK_THREADS + tid;
        live[j] = p < n_seg;
        cl[j] = __builtin_inff();
#pragma unroll
        for (int e = 0; e < K; ++e) v[j][e] = 0.f;
        if (live[j]) {
            const TokSeg g = tok_locate(st, c, p);
            tok_load<K>(st, c, g, v[j]);
            if (step >= 1) {
                const float d = tok_d2<K>(v[j], cc);
                if (step >= 2) cl[j] = closest[(int64_t)c * n_seg + p];
                cl[j] = d < cl[j] ? d : cl[j];           // (a NaN distance leaves what is there)
                closest[(int64_t)c * n_seg + p] = cl[j];
            }
        }
    }
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        float row[K];
#pragma unroll
        for (int e = 0; e < K; ++e) row[e] = cc[(t + 1) * K + e];
        u64 a = 0;
#pragma unroll
        for (int j = 0; j < SEED_PER; ++j) {
            const float d = tok_d2<K>(v[j], row);
            if (live[j]) a += tok_quant(d < cl[j] ? d : cl[j], F);
        }
        a = wave_sum_u64(a);
        if (lane == 0) red[wave][t] = a;
    }
    __syncthreads();
    if (tid < T) {
        u64 s = 0;
#pragma unroll
        for (int w = 0; w < TOK_THREADS / WAVE; ++w) s += red[w][tid];
        block_sums[(int64_t)tid * NB + (int64_t)c * gridDim.x + blockIdx.x] = s;
    }
}

template <int K>
__global__ __launch_bounds__(SEED_PICK_THREADS) void tok_seed_pick_kernel(TokStore st, int64_t n_seg, int64_t B, int64_t NB, int step, int T, int T_next,
                                                                           int n_trials, const u64 *__restrict__ u53, const float *__restrict__ closest,
                                                                           const u64 *__restrict__ block_sums, float *cand_c, int64_t *cand_g,
                                                                           float *__restrict__ centers, int64_t *__restrict__ indices,
                                                                           u64 *__restrict__ trace, const uint32_t *__restrict__ amax, int fbase) {
    __shared__ u64 wsum[SEED_PICK_THREADS / WAVE], pots[SEED_TMAX], tgt[SEED_TMAX], res[SEED_TMAX];
    __shared__ int64_t blk[SEED_TMAX];
    __shared__ float acc_c[K];
    __shared__ int s_win;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the potentials of the step's candidates
    for (int t = 0; t < T; ++t) {
        u64 a = 0;
        for (int64_t i = tid; i < NB; i += SEED_PICK_THREADS) a += block_sums[(int64_t)t * NB + i];
        a = wave_sum_u64(a);
        if (lane == 0) wsum[wave] = a;
        __syncthreads();
        if (tid == 0) {
            u64 s = 0;
            for (int w = 0; w < SEED_PICK_THREADS / WAVE; ++w) s += wsum[w];
            pots[t] = s;
        }
        __syncthreads();
    }
    if (tid == 0) {                                      // the smallest potential; equal potentials go to the smaller trial index
        int win = 0;
        for (int t = 1; t < T; ++t) win = pots[t] < pots[win] ? t : win;
        s_win = win;
        indices[step] = cand_g[win];
        if (trace && step >= 1) {
            for (int t = 0; t < T; ++t) {
                trace[((int64_t)(step - 1) * n_trials + t) * 2] = (u64)cand_g[t];
                trace[((int64_t)(step - 1) * n_trials + t) * 2 + 1] = pots[t];
            }
        }
    }
    __syncthreads();
    const int win = s_win;
    const u64 potw = pots[win];
    if (tid < K) {
        const float w = cand_c[win * K + tid];
        centers[(int64_t)step * K + tid] = w;
        acc_c[tid] = w;
    }
    if (T_next == 0) return;
    // the next step's targets, (U pot) >> 53 of the 117-bit product, and the workgroup of the sweep each falls into
    if (tid < T_next) {
        const u64 U = u53[tid];
        tgt[tid] = (__umul64hi(U, potw) << 11) | ((U * potw) >> 53);
        blk[tid] = 0;
        res[tid] = 0;
    }
    const u64 *__restrict__ bs = block_sums + (int64_t)win * NB;
    const int64_t chunk = (NB + SEED_PICK_THREADS - 1) / SEED_PICK_THREADS;
    const int64_t lo = tid * chunk < NB ? tid * chunk : NB, hi = lo + chunk < NB ? lo + chunk : NB;
    u64 cs = 0;
    for (int64_t i = lo; i < hi; ++i) cs += bs[i];
    const u64 incl = block_scan_u64(cs, wsum), excl = incl - cs;       // (its barriers also publish tgt and acc_c)
    for (int t = 0; t < T_next; ++t) {
        const u64 tg = tgt[t];
        if (tg >= excl && tg < incl) {                   // one thread: the chunks partition [0, pot) and tg < pot
            u64 run = excl;
            for (int64_t i = lo; i < hi; ++i) {
                const u64 b = bs[i];
                if (tg < run + b) { blk[t] = i; res[t] = tg - run; break; }
                run += b;
            }
        }
    }
    __syncthreads();
    // inside that span: the winner's weights again, by the sweep's expression, scanned to the first segment whose running sum exceeds the target
    const int F = tok_seed_f(fbase, *amax);
    for (int t = 0; t < T_next; ++t) {
        const int c = (int)(blk[t] / B);
        const int64_t p = (blk[t] % B) * SEED_SPAN + tid;
        float v[K];
#pragma unroll
        for (int e = 0; e < K; ++e) v[e] = 0.f;
        u64 qv = 0;
        if (p < n_seg) {
            const TokSeg g = tok_locate(st, c, p);
            tok_load<K>(st, c, g, v);
            const float d = tok_d2<K>(v, acc_c);
            const float cl = step >= 1 ? closest[(int64_t)c * n_seg + p] : __builtin_inff();
            qv = tok_quant(d < cl ? d : cl, F);
        }
        const u64 run = block_scan_u64(qv, wsum);
        const u64 r = res[t];
        const bool hit = potw ? (qv != 0 && run > r && run - qv <= r) : tid == 0;      // pot == 0: g = 0, what searchsorted returns there
        if (hit) {
            cand_g[t] = (int64_t)c * n_seg + p;
#pragma unroll
            for (int e = 0; e < K; ++e) cand_c[t * K + e] = v[e];
        }
    }
}

// =====================================================================================================
// decode: one thread per segment, written back in the store's layout and cut at the run's length
// =====================================================================================================
template <int K>
__global__ __launch_bounds__(TOK_THREADS) void tok_decode_kernel(TokStore st, float *__restrict__ out, int64_t n_seg, const int32_t *__restrict__ ids,
                                                                  const float *__restrict__ means, const float *__restrict__ centers, int V) {
    const int64_t p = (int64_t)blockIdx.x * TOK_THREADS + threadIdx.x;
    if (p >= n_seg) return;
    const int c = blockIdx.y;
    const TokSeg g = tok_locate(st, c, p);
    const int id = ids[g.dst];
    const bool ok = id >= 0 && id < V;
    const float m = means[g.dst];
    float *__restrict__ o = out + st.src_off[g.r] + (int64_t)c * st.lead_stride;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        const int64_t i = g.s * K + e;
        if (i < g.len) o[i] = ok ? centers[(int64_t)id * K + e] + m : __builtin_nanf("");
    }
}

// =====================================================================================================
// entry points
// =====================================================================================================
static inline bool tok_table_ok(int V) { return V >= 1 && V <= ECGVIT_TOK_MAX_CLUSTERS; }

int ecgvit_tok_assign(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, const float *centers, int V,
                      const int32_t *prev_ids, int32_t *ids, float *means, float *dist, uint64_t *changed, void *stream) {
    if (!tok_store_ok(x, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, pad) || !tok_table_ok(V) || !tok_al(centers, 4) || !tok_al(ids, 4) ||
        !tok_al(means, 4) || (dist && !tok_al(dist, 4)) || (prev_ids && !tok_al(prev_ids, 4)) || (changed && !tok_al(changed, 8)) ||
        (prev_ids == nullptr) != (changed == nullptr))
        return ECGVIT_EINVAL;
    const int64_t blocks = (n_seg + TOK_SPAN - 1) / TOK_SPAN;
    if (blocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
    if (changed && hipMemsetAsync(changed, 0, sizeof(uint64_t), as_stream(stream)) != hipSuccess) return ECGVIT_ELAUNCH;
    const TokStore st = tok_store(x, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, pad);
#define TOK_LAUNCH(KK)                                                                                                                       \
    hipLaunchKernelGGL(tok_assign_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, centers, V, prev_ids, ids, \
                       means, dist, reinterpret_cast<u64 *>(changed))
    TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int64_t ecgvit_tok_workspace(int V, int k) {
    if (!tok_table_ok(V) || !(k == 8 || k == 16 || k == 32)) return 0;
    return ((int64_t)V * k + V + 2) * 8;
}

int ecgvit_tok_update(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, const int32_t *ids,
                      float *centers, int V, int64_t *lens, void *workspace, int keep_amax, void *stream) {
    if (!tok_store_ok(x, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, pad) || !tok_table_ok(V) || !tok_al(ids, 4) || !tok_al(centers, 4) ||
        !tok_al(lens, 8) || !tok_al(workspace, 8) || (keep_amax != 0 && keep_amax != 1))
        return ECGVIT_EINVAL;
    if (n_seg > 0xFFFFFFFFll / C) return ECGVIT_EINVAL;   // C * n_seg >= 2^32: past what the fixed-point sums admit
    const int64_t blocks = (n_seg + TOK_THREADS - 1) / TOK_THREADS;
    if (blocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
    u64 *sums = reinterpret_cast<u64 *>(workspace), *counts = sums + (int64_t)V * k;
    uint32_t *amax = reinterpret_cast<uint32_t *>(counts + V);
    // the sums and the counts always; the maximum (the last 16 bytes) only when it is taken anew
    const size_t zero_bytes = (size_t)ecgvit_tok_workspace(V, k) - (keep_amax ? 16 : 0);
    if (hipMemsetAsync(workspace, 0, zero_bytes, as_stream(stream)) != hipSuccess) return ECGVIT_ELAUNCH;
    const TokStore st = tok_store(x, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, pad);
    if (!keep_amax) {   // the maximum depends on the store alone, not on ids: one sweep serves every update of a fit
#define TOK_LAUNCH(KK) hipLaunchKernelGGL(tok_amax_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, amax)
        TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
        ECGVIT_CHECK_LAUNCH();
    }
#define TOK_LAUNCH(KK) \
    hipLaunchKernelGGL(tok_accum_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, ids, V, amax, sums, counts)
    TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
    ECGVIT_CHECK_LAUNCH();
    hipLaunchKernelGGL(tok_finish_kernel, dim3((V * k + TOK_THREADS - 1) / TOK_THREADS), dim3(TOK_THREADS), 0, as_stream(stream), sums, counts, amax, V, k,
                       centers, lens);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

static inline bool tok_seed_shape_ok(int C, int64_t n_seg, int V, int k, int n_trials) {
    return tok_table_ok(V) && (k == 8 || k == 16 || k == 32) && C >= 1 && C <= 65535 && n_seg >= 1 && n_trials >= 1 && n_trials <= SEED_TMAX &&
           n_seg <= 0xFFFFFFFFll / C && (int64_t)V <= (int64_t)C * n_seg;      // C * n_seg >= 2^32: past what the integer potentials admit
}

int64_t ecgvit_tok_seed_workspace(int C, int64_t n_seg, int V, int k, int n_trials) {
    if (!tok_seed_shape_ok(C, n_seg, V, k, n_trials)) return 0;
    const int64_t NB = (n_seg + SEED_SPAN - 1) / SEED_SPAN * C;
    return SEED_WS_SUMS + (int64_t)n_trials * NB * 8 + (((int64_t)C * n_seg * 4 + 7) & ~7ll);
}

int ecgvit_tok_seed(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                    const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, int V, int n_trials, int64_t first,
                    const uint64_t *u53, float *centers, int64_t *indices, uint64_t *trace, void *workspace, int keep_amax, void *stream) {
    if (!tok_store_ok(x, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, pad) || !tok_seed_shape_ok(C, n_seg, V, k, n_trials) ||
        first < 0 || first >= (int64_t)C * n_seg || (V > 1 && !tok_al(u53, 8)) || !tok_al(centers, 4) || !tok_al(indices, 8) ||
        (trace && !tok_al(trace, 8)) || !tok_al(workspace, 8) || (keep_amax != 0 && keep_amax != 1))
        return ECGVIT_EINVAL;
    const int64_t B = (n_seg + SEED_SPAN - 1) / SEED_SPAN, NB = B * C, ablocks = (n_seg + TOK_THREADS - 1) / TOK_THREADS;
    if (ablocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
    char *ws = reinterpret_cast<char *>(workspace);
    uint32_t *amax = reinterpret_cast<uint32_t *>(ws);
    int64_t *cand_g = reinterpret_cast<int64_t *>(ws + SEED_WS_CAND_G);
    float *cand_c = reinterpret_cast<float *>(ws + SEED_WS_CAND_C);
    u64 *block_sums = reinterpret_cast<u64 *>(ws + SEED_WS_SUMS);
    float *closest = reinterpret_cast<float *>(block_sums + (int64_t)n_trials * NB);
    int H = 0, log2k = 0;
    while (((int64_t)C * n_seg) >> H) ++H;               // bit_length(C * n_seg)
    while ((1 << log2k) < k) ++log2k;
    const int fbase = 63 - H - 2 - log2k;
    const TokStore st = tok_store(x, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, pad);
    if (!keep_amax) {
        if (hipMemsetAsync(amax, 0, 16, as_stream(stream)) != hipSuccess) return ECGVIT_ELAUNCH;
#define TOK_LAUNCH(KK) hipLaunchKernelGGL(tok_amax_kernel<KK>, dim3((unsigned)ablocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, amax)
        TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
        ECGVIT_CHECK_LAUNCH();
    }
    for (int s = 0; s < V; ++s) {
        const int T = s ? n_trials : 1, T_next = s + 1 < V ? n_trials : 0;
        const u64 *u = T_next ? reinterpret_cast<const u64 *>(u53) + (int64_t)s * n_trials : nullptr;
#define TOK_LAUNCH(KK)                                                                                                                          \
    hipLaunchKernelGGL(tok_seed_sweep_kernel<KK>, dim3((unsigned)B, C), dim3(TOK_THREADS), 0, as_stream(stream), st, n_seg, s, T, first, centers, \
                       cand_c, cand_g, closest, block_sums, NB, amax, fbase)
        TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
        ECGVIT_CHECK_LAUNCH();
#define TOK_LAUNCH(KK)                                                                                                                      \
    hipLaunchKernelGGL(tok_seed_pick_kernel<KK>, dim3(1), dim3(SEED_PICK_THREADS), 0, as_stream(stream), st, n_seg, B, NB, s, T, T_next, n_trials, \
                       u, closest, block_sums, cand_c, cand_g, centers, indices, reinterpret_cast<u64 *>(trace), amax, fbase)
        TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
        ECGVIT_CHECK_LAUNCH();
    }
    return ECGVIT_OK;
}

int ecgvit_tok_decode(float *out,const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, const int32_t *ids, const float *means,
                      const float *centers, int V, void *stream) {
    if (!tok_store_ok(out, src_off, raw_len, seg_cum, dst_off, R, C, n_seg, k, 0) || !tok_table_ok(V) || !tok_al(ids, 4) || !tok_al(means, 4) ||
        !tok_al(centers, 4))
        return ECGVIT_EINVAL;
    const int64_t blocks = (n_seg + TOK_THREADS - 1) / TOK_THREADS;
    if (blocks > 0x7FFFFFFFll) return ECGVIT_EINVAL;
    const TokStore st = tok_store(out, src_off, lead_stride, raw_len, seg_cum, dst_off, dst_stride, R, 0);
#define TOK_LAUNCH(KK) \
    hipLaunchKernelGGL(tok_decode_kernel<KK>, dim3((unsigned)blocks, C), dim3(TOK_THREADS), 0, as_stream(stream), st, out, n_seg, ids, means, centers, V)
    TOK_BY_K(k, TOK_LAUNCH);
#undef TOK_LAUNCH
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
