// The fused bf16 attention that is not the tuned dh = 64 full-row path of attention.hip, from one kernel text (attn_varlen_kernels.h) in three
// forms: the uniform batch at dh = 128 (ecgvit_attention_fwd / _bwd call attn_fwd_run / attn_bwd_run) and the CLS-row kernels at dh = 64 and
// 128 (ecgvit_attention_cls_*); variable-length records (ecgvit_attention_varlen_*); ragged batches (ecgvit_attention_ragged_*).  Also the f32
// path's masked row softmax and the patch gather that zeroes the patches past each record's length (ecgvit_softmax_rows_varlen /
// ecgvit_patch_gather_varlen).
//
// Templated on HI, the number of 64-wide head images (1: dh = 64, 2: dh = 128): every [row][64 HI x bf16] operand sits in LDS as HI standard
// [row][64] images (attn_common.h swizzle and fragment readers).
// forward   one 4-wave workgroup per (record, head, 128-query block); each wave owns 32 queries (query on the lane), online softmax over 64-key
//           windows of K and V staged in LDS (S^T = K Q^T, O^T += V^T P^T, lazy running maximum as in attention.hip).
// backward  two kernels, deterministic without atomics: dK / dV per 128-key block (key on the lane, loop over 32-query blocks of Q / dO staged
//           in LDS, the 2 HI dK^T / dV^T accumulators in registers) and dQ per 128-query block (P recomputed from the stored LSE).
// CLS row   VALU kernels for query row 0 only (the pruned last block of the supervised step).
//
// Variable-length records: a batch keeps one row stride N (the widest record); record b holds n_tok[b] valid tokens, 1 <= n_tok[b] <= N, read
// once per workgroup as a scalar.  Key loops end at n_tok[b] (the ragged last window masks keys >= n_tok[b] as the uniform form masks keys
// >= N), query / key blocks that lie entirely past n_tok[b] only zero-fill, and rows >= n_tok[b] of out and of all three parts of dqkv are
// written as exact zeros: the padded rows then add exactly 0 to every weight gradient, and a record's valid outputs do not depend on what its
// padded rows of qkv hold.  The LSE of a padded row is 0.
// Ragged batches: record b owns rows [tok_off[b], tok_off[b] + n_tok[b]) -- the records' tokens follow one another with no padded rows, so
// nothing past n_tok[b] is read or written (no zero-fill).  N is then the widest record's token count: it sets the grid, the LSE layout
// (bh N + q) and the dropout hashing, which are therefore those of the padded pass on the valid region.
// Contract shared with attention.hip's kernels: same qkv / out / lse / dqkv layouts, LSE = m scale + log(sum p) in natural-log units, the
// same dropout bits indexed with the batch N -- element (bh, q, key): quad = (bh N + q) ceil(N / 4) + key / 4, byte key & 3, keep iff
// byte >= round(256 p), kept values scaled by 256 / (256 - round(256 p)) -- so the mask of the valid region is what the uniform kernel draws.
// No atomics: every output element is written by exactly one lane, so launches are bit-reproducible.
#include "attn_common.h"

namespace {

constexpr int AV_WK = 64;   // keys per K / V window (forward, dQ)
constexpr float AV_LOG2E = 1.44269504088896340736f;

// vector phase of one 32-key x 32-query score tile with 2 HI output accumulators: lazy running maximum (moves only when a tile exceeds it by
// more than 2^8), p = exp2(s c - m c), row sum, dropout, bf16 pairs
template <int HI, bool DROP>
__device__ __forceinline__ void av_tile_vec(f32x16 &sc, float &m, float &l, f32x16 (&o)[2 * HI], float c, uint32_t smix, uint32_t quad0,
                                            uint32_t thresh, u32x4 (&pk)[2]) {
    float mx = sc[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, sc[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__any((mx - m) * c > 8.0f)) {   // wave-uniform; always taken on the first tile (m = -inf, key 0 is valid)
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * c);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
    }
    const float mc = m * c;
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float p = __builtin_amdgcn_exp2f(fmaf(sc[r], c, -mc));
        sc[r] = p;
        ls += p;
    }
    l += ls;
    if constexpr (DROP) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t hh = quad_hash(smix, quad0 + (uint32_t)(2 * g));
#pragma unroll
            for (int k = 0; k < 4; ++k) sc[4 * g + k] = ((hh >> (8 * k)) & 0xFFu) >= thresh ? sc[4 * g + k] : 0.f;
        }
    }
#pragma unroll
    for (int ss = 0; ss < 2; ++ss) pk[ss] = __builtin_bit_cast(u32x4, pack8(sc, ss));
}

// one 8-byte store of accumulator values 4 g .. 4 g + 3 (rows 8 g + 4 lh + 0..3 of a 32-row block), times f
__device__ __forceinline__ void av_store4(bf16_t *dst, const f32x16 &acc, int g, float f) {
    bf16x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (bf16_t)(acc[4 * g + k] * f);
    *reinterpret_cast<bf16x4 *>(dst) = v;
}
__device__ __forceinline__ void av_zero4(bf16_t *dst) { *reinterpret_cast<u32x2 *>(dst) = u32x2{0u, 0u}; }


// zero rows [r0, r1) x DH of `dst` (row stride ld elements) with the whole workgroup, 16 B per store
template <int DH>
__device__ __forceinline__ void av_zero_rows(bf16_t *dst, int64_t ld, int r0, int r1) {
    constexpr int CH = DH / 8;
    for (int c = threadIdx.x; c < (r1 - r0) * CH; c += 256) {
        const int row = r0 + c / CH, ch = c % CH;
        *reinterpret_cast<u32x4 *>(dst + (int64_t)row * ld + ch * 8) = u32x4{0u, 0u, 0u, 0u};
    }
}

constexpr int AVC_NMAX = ECGVIT_ATTN_MAX_N;
template <int HI> __device__ __forceinline__ float avc_group_sum(float v) {   // sum over the 8 HI lanes that share a key slot
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    if constexpr (HI == 2) v += __shfl_xor(v, 8, 64);
    return v;
}
template <bool DROP> __device__ __forceinline__ float avc_mult(uint32_t smix, uint32_t quad0, int key, uint32_t thresh, float inv_keep) {
    if constexpr (!DROP) return 1.f;
    const uint32_t hsh = quad_hash(smix, quad0 + (uint32_t)(key >> 2));
    return ((hsh >> (8 * (key & 3))) & 0xFFu) >= thresh ? inv_keep : 0.f;
}
template <bool MAX> __device__ __forceinline__ float avc_block_reduce(float v, float *red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}


#define AV_FORM 0
#include "attn_varlen_kernels.h"
#undef AV_FORM
#define AV_FORM 1
#include "attn_varlen_kernels.h"
#undef AV_FORM
#define AV_FORM 2
#include "attn_varlen_kernels.h"
#undef AV_FORM

// =====================================================================================================
// f32 parity path: in-place row softmax of the scores S[(b h + head) N + q][ld] over the first n_tok[b] columns; columns >= n_tok[b] and
// every column of the rows q >= n_tok[b] become 0 (ecgvit_softmax_bwd_rows then gives dS = 0 there).  One wave per row.
// =====================================================================================================
__global__ __launch_bounds__(256) void softmax_rows_varlen_kernel(float *__restrict__ S, const int32_t *__restrict__ n_tok, int64_t rows, int hN,
                                                                 int N, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4ll + (threadIdx.x >> 6), nw = gridDim.x * 4ll;
    for (int64_t r = wave0; r < rows; r += nw) {
        float *s = S + r * ld;
        const int nb = n_tok[r / hN], q = (int)(r % N);
        if (q >= nb) {
            for (int c = lane; c < N; c += 64) s[c] = 0.f;
            continue;
        }
        float m = -INFINITY;
        for (int c = lane; c < nb; c += 64) m = fmaxf(m, s[c]);
        m = wave_max(m);
        float sum = 0.f;
        for (int c = lane; c < nb; c += 64) sum += expf(s[c] - m);
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int c = lane; c < N; c += 64) s[c] = c < nb ? expf(s[c] - m) * inv : 0.f;
    }
}

// =====================================================================================================
// patch Rearrange with per-record lengths: patches[b n + j][f] = x[b][c][j P + s] (f = s C + c) for j < n_tok[b] - 1, 0 past it and for the
// row padding f >= C P.  Samples past a record's length are never read.
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void patch_gather_varlen_kernel(const float *__restrict__ x, T *__restrict__ out, const int32_t *__restrict__ n_tok,
                                                                  int C, int L, int P, int n, int64_t ld) {
    const int b = blockIdx.y;
    const int np = n_tok[b] - 1;
    const int CP = C * P;
    const int64_t total = (int64_t)n * ld;
    const float *xb = x + (int64_t)b * C * L;
    T *ob = out + (int64_t)b * total;
    for (int64_t idx = blockIdx.x * 256ll + threadIdx.x; idx < total; idx += gridDim.x * 256ll) {
        const int j = (int)(idx / ld), f = (int)(idx - (int64_t)j * ld);
        float v = 0.f;
        if (j < np && f < CP) {
            const int s = f / C, c = f - s * C;
            v = xb[(int64_t)c * L + (int64_t)j * P + s];
        }
        ob[idx] = from_f32<T>(v);
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// One launcher per operation for the three forms: n_tok == nullptr -> uniform (attnu_*), tok_off == nullptr -> padded (attnv_*), else packed
// (attnr_*).  Each checks what every entry point of the operation checks, then launches K<HI, DROP> for dh = 64 HI and the dropout threshold.
// The uniform fwd / bwd serve dh = 128 only (the dh = 128 branches of ecgvit_attention_fwd / _bwd): dh = 64 runs the tuned kernels of attention.hip.
static bool attn_args_ok(int B, int N, int h, int dh, float dropout_p) {
    if ((dh != 64 && dh != 128) || N < 1 || N > ECGVIT_ATTN_MAX_N || B < 1 || h < 1) return false;
    return !(dropout_p > 0.f && dropout_threshold8(dropout_p) == 0);   // p < 1/512 would silently round to no dropout
}
static bool attn_grid_ok(int B, int N, int h) { return (int64_t)B * h * ((N + 127) / 128) < (1ll << 31); }   // the fwd / bwd grid
static bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

#define AV_DROP(K, HI, G, ...)                                                                                  \
    do {                                                                                                        \
        if (th) hipLaunchKernelGGL((K<HI, true>), G, dim3(256), 0, as_stream(stream), __VA_ARGS__);           \
        else hipLaunchKernelGGL((K<HI, false>), G, dim3(256), 0, as_stream(stream), __VA_ARGS__);             \
    } while (0)
#define AV_HI_DROP(K, G, ...)                                          \
    do {                                                               \
        if (dh == 64) AV_DROP(K, 1, G, __VA_ARGS__);                   \
        else AV_DROP(K, 2, G, __VA_ARGS__);                            \
    } while (0)

int attn_fwd_run(const void *qkv, void *out, float *lse, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h, int dh, float scale,
                 float dropout_p, uint64_t seed, void *stream) {
    if (!attn_args_ok(B, N, h, dh, dropout_p) || !attn_grid_ok(B, N, h) || (!n_tok && dh != 128) || !aligned16(qkv) || !aligned16(out))
        return ECGVIT_EINVAL;
    const uint32_t th = dropout_threshold8(dropout_p);
    const float ik = dropout_inv_keep8(dropout_p);
    const dim3 grid((unsigned)(B * h * ((N + 127) / 128)));
    const bf16_t *q = (const bf16_t *)qkv;
    bf16_t *o = (bf16_t *)out;
    if (!n_tok) AV_DROP(attnu_fwd_kernel, 2, grid, q, o, lse, N, h, scale, seed, th, ik);
    else if (!tok_off) AV_HI_DROP(attnv_fwd_kernel, grid, q, o, lse, n_tok, N, h, scale, seed, th, ik);
    else AV_HI_DROP(attnr_fwd_kernel, grid, q, o, lse, n_tok, tok_off, N, h, scale, seed, th, ik);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int attn_bwd_run(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, const int32_t *n_tok, const int32_t *tok_off,
                 int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!attn_args_ok(B, N, h, dh, dropout_p) || !attn_grid_ok(B, N, h) || (!n_tok && dh != 128) || !aligned16(qkv) || !aligned16(out) ||
        !aligned16(dout) || !aligned16(dqkv))
        return ECGVIT_EINVAL;
    const uint32_t th = dropout_threshold8(dropout_p);
    const float ik = dropout_inv_keep8(dropout_p);
    const dim3 grid((unsigned)(B * h * ((N + 127) / 128)));   // 128-key blocks (dK / dV) = 128-query blocks (dQ)
    const bf16_t *q = (const bf16_t *)qkv, *o = (const bf16_t *)out, *dO = (const bf16_t *)dout;
    bf16_t *dq = (bf16_t *)dqkv;
    if (!n_tok) AV_DROP(attnu_bwd_dkv_kernel, 2, grid, q, o, dO, lse, dq, N, h, scale, seed, th, ik);
    else if (!tok_off) AV_HI_DROP(attnv_bwd_dkv_kernel, grid, q, o, dO, lse, dq, n_tok, N, h, scale, seed, th, ik);
    else AV_HI_DROP(attnr_bwd_dkv_kernel, grid, q, o, dO, lse, dq, n_tok, tok_off, N, h, scale, seed, th, ik);
    ECGVIT_CHECK_LAUNCH();
    if (!n_tok) AV_DROP(attnu_bwd_dq_kernel, 2, grid, q, o, dO, lse, dq, N, h, scale, seed, th, ik);
    else if (!tok_off) AV_HI_DROP(attnv_bwd_dq_kernel, grid, q, o, dO, lse, dq, n_tok, N, h, scale, seed, th, ik);
    else AV_HI_DROP(attnr_bwd_dq_kernel, grid, q, o, dO, lse, dq, n_tok, tok_off, N, h, scale, seed, th, ik);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

// (the padded / packed CLS entry points have always held B h to the fwd / bwd grid limit as well)
static int attn_cls_fwd_run(const void *qkv, void *out_cls, float *lse_cls, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h,
                            int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!attn_args_ok(B, N, h, dh, dropout_p) || (int64_t)B * h >= (1ll << 31) || (n_tok && !attn_grid_ok(B, N, h)) || !aligned16(qkv) ||
        !aligned16(out_cls))
        return ECGVIT_EINVAL;
    const uint32_t th = dropout_threshold8(dropout_p);
    const float ik = dropout_inv_keep8(dropout_p);
    const dim3 grid((unsigned)(B * h));
    const bf16_t *q = (const bf16_t *)qkv;
    bf16_t *o = (bf16_t *)out_cls;
    if (!n_tok) AV_HI_DROP(attnu_cls_fwd_kernel, grid, q, o, lse_cls, N, h, scale, seed, th, ik);
    else if (!tok_off) AV_HI_DROP(attnv_cls_fwd_kernel, grid, q, o, lse_cls, n_tok, N, h, scale, seed, th, ik);
    else AV_HI_DROP(attnr_cls_fwd_kernel, grid, q, o, lse_cls, n_tok, tok_off, N, h, scale, seed, th, ik);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

static int attn_cls_bwd_run(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls,
                            const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed,
                            void *stream) {
    if (!attn_args_ok(B, N, h, dh, dropout_p) || (int64_t)B * h >= (1ll << 31) || (n_tok && !attn_grid_ok(B, N, h)) || !aligned16(qkv) ||
        !aligned16(out_cls) || !aligned16(dout_cls) || !aligned16(dqkv) || !aligned16(dq_cls))
        return ECGVIT_EINVAL;
    const uint32_t th = dropout_threshold8(dropout_p);
    const float ik = dropout_inv_keep8(dropout_p);
    const dim3 grid((unsigned)(B * h));
    const bf16_t *q = (const bf16_t *)qkv, *o = (const bf16_t *)out_cls, *dO = (const bf16_t *)dout_cls;
    bf16_t *dk = (bf16_t *)dqkv, *dq = (bf16_t *)dq_cls;
    if (!n_tok) AV_HI_DROP(attnu_cls_bwd_kernel, grid, q, o, dO, lse_cls, dk, dq, N, h, scale, seed, th, ik);
    else if (!tok_off) AV_HI_DROP(attnv_cls_bwd_kernel, grid, q, o, dO, lse_cls, dk, dq, n_tok, N, h, scale, seed, th, ik);
    else AV_HI_DROP(attnr_cls_bwd_kernel, grid, q, o, dO, lse_cls, dk, dq, n_tok, tok_off, N, h, scale, seed, th, ik);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
#undef AV_HI_DROP
#undef AV_DROP

extern "C" {

int ecgvit_attention_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed,
                             int dtype, void *stream) {
    if (dtype != ECGVIT_BF16 || !qkv || !out_cls || !lse_cls) return ECGVIT_EINVAL;
    return attn_cls_fwd_run(qkv, out_cls, lse_cls, nullptr, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls, int B, int N,
                             int h, int dh, float scale, float dropout_p, uint64_t seed, int dtype, void *stream) {
    if (dtype != ECGVIT_BF16 || !qkv || !out_cls || !dout_cls || !lse_cls || !dqkv || !dq_cls) return ECGVIT_EINVAL;
    return attn_cls_bwd_run(qkv, out_cls, dout_cls, lse_cls, dqkv, dq_cls, nullptr, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_varlen_fwd(const void *qkv, void *out, float *lse, const int32_t *n_tok, int B, int N, int h, int dh, float scale,
                                float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok) return ECGVIT_EINVAL;
    return attn_fwd_run(qkv, out, lse, n_tok, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_varlen_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, const int32_t *n_tok, int B, int N,
                                int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok) return ECGVIT_EINVAL;
    return attn_bwd_run(qkv, out, dout, lse, dqkv, n_tok, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_varlen_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, const int32_t *n_tok, int B, int N, int h, int dh, float scale,
                                    float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok) return ECGVIT_EINVAL;
    return attn_cls_fwd_run(qkv, out_cls, lse_cls, n_tok, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_varlen_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls,
                                    const int32_t *n_tok, int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok) return ECGVIT_EINVAL;
    return attn_cls_bwd_run(qkv, out_cls, dout_cls, lse_cls, dqkv, dq_cls, n_tok, nullptr, B, N, h, dh, scale, dropout_p, seed, stream);
}

// ragged batch: record b's rows start at tok_off[b] (int32 [B] on the device, with n_tok); N = the widest record's token count
int ecgvit_attention_ragged_fwd(const void *qkv, void *out, float *lse, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h, int dh,
                                float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok || !tok_off) return ECGVIT_EINVAL;
    return attn_fwd_run(qkv, out, lse, n_tok, tok_off, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_ragged_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, const int32_t *n_tok,
                                const int32_t *tok_off, int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok || !tok_off) return ECGVIT_EINVAL;
    return attn_bwd_run(qkv, out, dout, lse, dqkv, n_tok, tok_off, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_ragged_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h,
                                    int dh, float scale, float dropout_p, uint64_t seed, void *stream) {
    if (!n_tok || !tok_off) return ECGVIT_EINVAL;
    return attn_cls_fwd_run(qkv, out_cls, lse_cls, n_tok, tok_off, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_attention_ragged_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls,
                                    const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h, int dh, float scale, float dropout_p,
                                    uint64_t seed, void *stream) {
    if (!n_tok || !tok_off) return ECGVIT_EINVAL;
    return attn_cls_bwd_run(qkv, out_cls, dout_cls, lse_cls, dqkv, dq_cls, n_tok, tok_off, B, N, h, dh, scale, dropout_p, seed, stream);
}

int ecgvit_softmax_rows_varlen(float *S, const int32_t *n_tok, int B, int h, int N, int64_t ld, void *stream) {
    if (B <= 0 || h <= 0 || N <= 0 || ld < N || !n_tok) return ECGVIT_EINVAL;
    const int64_t rows = (int64_t)B * h * N;
    const int grid = (int)std::min<int64_t>((rows + 3) / 4, 2048);
    hipLaunchKernelGGL(softmax_rows_varlen_kernel, dim3(grid), dim3(256), 0, as_stream(stream), S, n_tok, rows, h * N, N, ld);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_patch_gather_varlen(const float *x, void *patches, const int32_t *n_tok, int B, int C, int L, int P, int64_t ld, int dtype, void *stream) {
    if (B <= 0 || C <= 0 || P <= 0 || L <= 0 || L % P != 0 || ld < (int64_t)C * P || !n_tok || B > 65535) return ECGVIT_EINVAL;
    const int n = L / P;
    const int64_t per = (int64_t)n * ld;
    const dim3 grid((unsigned)std::min<int64_t>((per + 255) / 256, 1024), (unsigned)B);
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        hipLaunchKernelGGL(patch_gather_varlen_kernel<T>, grid, dim3(256), 0, as_stream(stream), x, (T *)patches, n_tok, C, L, P, n, ld);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

}  // extern "C"
