// What every kernel over the tokenizer's segments shares (tokenize.hip, dbscan.hip): the store's address tables, the segment load with the
// padding applied inside it, the unfused f32 squared distance, and the launchers' argument checks.  Contract: include/ecgvit_hip.h.
#pragma once
#include "common.h"

#define TOK_THREADS 256

typedef unsigned long long u64;

struct TokStore {
    const float *x;
    const int64_t *src_off;
    int64_t lead_stride;
    const int32_t *raw_len;
    const int64_t *seg_cum;
    const int64_t *dst_off;
    int64_t dst_stride;
    int R, pad;
};

// the record of position p: the last r with seg_cum[r] <= p (seg_cum[0] = 0 <= p < seg_cum[R])
__device__ __forceinline__ int tok_record(const int64_t *__restrict__ seg_cum, int R, int64_t p) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_cum[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

struct TokSeg { int r, len; int64_t s, dst; };

__device__ __forceinline__ TokSeg tok_locate(const TokStore &st, int c, int64_t p) {
    TokSeg g;
    g.r = tok_record(st.seg_cum, st.R, p);
    g.s = p - st.seg_cum[g.r];
    g.len = st.raw_len[g.r];
    g.dst = st.dst_off[g.r] + (int64_t)c * st.dst_stride + g.s;
    return g;
}

// the K samples of a segment minus their mean -> v, returns the mean.  Every index read lies in [0, len): position i >= len is 0 ('zero')
// or sample i - n_pad ('shift'), clamped into the run.
template <int K> __device__ __forceinline__ float tok_load(const TokStore &st, int c, const TokSeg &g, float (&v)[K]) {
    const float *__restrict__ base = st.x + st.src_off[g.r] + (int64_t)c * st.lead_stride;
    const int64_t len = g.len, i0 = g.s * K;
    const int64_t n_pad = K - (len % K);
#pragma unroll
    for (int e = 0; e < K; ++e) {
        const int64_t i = i0 + e;
        float t = 0.f;
        if (len > 0) {
            if (i < len) {
                t = base[i];
            } else if (st.pad == 1) {
                int64_t j = i - n_pad;
                j = j < 0 ? 0 : (j >= len ? len - 1 : j);
                t = base[j];
            }
        }
        v[e] = t;
    }
    float sum = v[0];
#pragma unroll
    for (int e = 1; e < K; ++e) sum = sum + v[e];
    const float mean = sum * (1.0f / K);
#pragma unroll
    for (int e = 0; e < K; ++e) v[e] = v[e] - mean;
    return mean;
}

// sum_e (s_e - c_e)^2: f32, UNFUSED (every difference, product and addition rounds on its own), in sample order
template <int K> __device__ __forceinline__ float tok_d2(const float (&v)[K], const float *c) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        const float d = v[e] - c[e];
        const float sq = d * d;
        acc = e ? acc + sq : sq;
    }
    return acc;
}

// ---- the seedings' integer weights (tokenize.hip, tok_scalable.hip) -------------------------------------
// 2^(31 - E) with 2^(E - 1) <= A < 2^E for the maximum's bit pattern (A = 0: any scale does)
__device__ __forceinline__ int tok_shift(uint32_t amax_bits) {
    const int ex = (int)(amax_bits >> 23);                 // biased exponent; 0 for a denormal maximum, 255 for inf / NaN
    return 31 - ((ex ? ex : 1) - 127 + 1);
}

// rint(d 2^F) in f64, where the product is exact; a non-finite distance (a segment with a non-finite sample, the untouched +inf) weighs nothing
__device__ __forceinline__ u64 tok_quant(float d, int F) {
    return (__float_as_uint(d) & 0x7F800000u) == 0x7F800000u ? 0ull : __double2ull_rn(ldexp((double)d, F));
}

// F = 63 - H - (2 E + 2 + log2 k) from fbase = 63 - H - 2 - log2 k and the maximum's bits
__device__ __forceinline__ int tok_seed_f(int fbase, uint32_t amax_bits) { return fbase - 2 * (31 - tok_shift(amax_bits)); }

// (U pot) >> 53 of the 117-bit product, U < 2^53
__device__ __forceinline__ u64 tok_target(u64 U, u64 pot) { return (__umul64hi(U, pot) << 11) | ((U * pot) >> 53); }

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive scan over the workgroup's threads in thread order; sh: one u64 per wave
__device__ __forceinline__ u64 block_scan_u64(u64 v, u64 *sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u64 before = 0;
    for (int w = 0; w < nw; ++w) before += w < wave ? sh[w] : 0ull;
    __syncthreads();
    return v + before;
}

// ---- the launchers' side -------------------------------------------------------------------------------
// the sweep for the absolute maximum of the mean-removed samples (tokenize.hip): *amax, zeroed by the caller, receives its bits
int tok_launch_amax(const struct TokStore &st, int C, int64_t n_seg, int k, uint32_t *amax, hipStream_t stream);
// fbase = 63 - H - 2 - log2 k with H = bit_length(C * n_seg): what tok_seed_f takes
static inline int tok_seed_fbase(int C, int64_t n_seg, int k) {
    int H = 0, log2k = 0;
    while (((int64_t)C * n_seg) >> H) ++H;
    while ((1 << log2k) < k) ++log2k;
    return 63 - H - 2 - log2k;
}

static inline bool tok_al(const void *p, unsigned a) { return p && (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

static bool tok_store_ok(const float *x, const int64_t *src_off, const int32_t *raw_len, const int64_t *seg_cum, const int64_t *dst_off, int R, int C,
                         int64_t n_seg, int k, int pad) {
    return tok_al(x, 4) && tok_al(src_off, 8) && tok_al(raw_len, 4) && tok_al(seg_cum, 8) && tok_al(dst_off, 8) && R >= 1 && C >= 1 && C <= 65535 &&
           n_seg >= (int64_t)R && (k == 8 || k == 16 || k == 32) && (pad == 0 || pad == 1);
}

static inline TokStore tok_store(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                                 const int64_t *dst_off, int64_t dst_stride, int R, int pad) {
    TokStore st;
    st.x = x; st.src_off = src_off; st.lead_stride = lead_stride; st.raw_len = raw_len; st.seg_cum = seg_cum; st.dst_off = dst_off;
    st.dst_stride = dst_stride; st.R = R; st.pad = pad;
    return st;
}

#define TOK_BY_K(k, launch)                      \
    do {                                         \
        if ((k) == 8) { launch(8); }             \
        else if ((k) == 16) { launch(16); }      \
        else { launch(32); }                     \
    } while (0)
