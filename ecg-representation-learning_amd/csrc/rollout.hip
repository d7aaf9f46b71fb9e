// Attention rollout for whole batches (EcgVit.attention_rollout_batch): the CLS-to-patch attention map of the reference's visualiser
// (ecg_vit.py:164-194) without ever holding an N x N matrix.  With A_i = mean_head P_i and the row sums of A_i + I taken as exactly 2:
//   c_i[k] = (A_i[0,k] + [k == 0]) / 2                               ecgvit_rollout_cls     (one query row per record and head)
//   r_i[k] = (sum_q c_i[q] A_{i-1}[q,k] + c_i[k]) / 2                ecgvit_rollout_colsum  (a weighted column sum of layer i-1's P)
//   map[i][k-1] = r_i[k] / max_{i, k >= 1} r_i[k]                    ecgvit_rollout_finish
// bf16: P is rebuilt tile by tile from the qkv / lse a fused forward left behind -- memory O(B h N), never O(B h N^2); f32: P is the
// materialised probs [B,h,N,N] of the parity path.  The three row layouts (uniform, n_tok, n_tok + tok_off) run the SAME kernel: the
// layout is two pointers that are NULL or not, read once per workgroup as scalars.
//
// Determinism: no atomics.  The weighted column sum of one (record, head) is one workgroup's loop over the record's query tiles in rising
// order (every tile's rows added in one fixed order); the h head sums meet in `workspace` ([B,h,N] f32) and a second launch adds them in head
// order.  The order of every output element is thus a function of the record's own n_b and of h alone: a record gives the same bits in a
// padded, a n_tok and a packed batch, alone or among others (what ecgvit_pool_records guarantees for pooling).
// Rows q >= n_b and keys k >= n_b are never read as data: their tile rows are zero-filled, their weights and lse taken as 0.
#include "attn_common.h"

namespace {

constexpr float RO_LOG2E = 1.44269504088896340736f;
constexpr int RO_QT = 64;   // queries per staged Q tile (two 32-row score tiles)

// tokens of record b (clamped into [0, N]: c / w / r rows hold N entries) and its first token row
__device__ __forceinline__ int ro_tokens(const int32_t *n_tok, int b, int N) { return n_tok ? max(0, min(n_tok[b], N)) : N; }
__device__ __forceinline__ int64_t ro_row0(const int32_t *tok_off, int b, int N) { return tok_off ? (int64_t)tok_off[b] : (int64_t)b * N; }

template <int HI> __device__ __forceinline__ float ro_group_sum(float v) {   // sum over the 8 HI lanes that share a key slot
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    if constexpr (HI == 2) v += __shfl_xor(v, 8, 64);
    return v;
}

// =====================================================================================================
// c[b,k] = (mean_head P[b,head,0,k] + [k == 0]) / 2, bf16: query row 0 of every head against the record's keys.  One workgroup per (record,
// chunk of 256 / (8 HI) keys): 8 HI lanes of 8 dims per key (one 16-B load per key row and head), heads added in rising order.  A bandwidth
// kernel as the CLS-row attention: N h dh products per record, no MFMA.
// =====================================================================================================
template <int HI>
__global__ __launch_bounds__(256) void rollout_cls_kernel(const bf16_t *__restrict__ qkv, const float *__restrict__ lse, float *__restrict__ c,
                                                          const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off, int N, int h,
                                                          float scale, int nchunk) {
    constexpr int DH = 64 * HI, G = 8 * HI, SLOTS = 256 / G;
    const int b = blockIdx.x / nchunk, k = (blockIdx.x - b * nchunk) * SLOTS + (int)threadIdx.x / G;
    const int g = threadIdx.x % G;
    const int n = ro_tokens(n_tok, b, N);
    if (n == 0) {
        if (g == 0 && k < N) c[(int64_t)b * N + k] = 0.f;
        return;
    }
    const int64_t dm = (int64_t)h * DH, ld = 3 * dm;
    const bf16_t *rec = qkv + ro_row0(tok_off, b, N) * ld + g * 8;
    const int kc = k < n ? k : n - 1;   // (keys >= n: clamped loads, zeros stored)
    float acc = 0.f;
    for (int head = 0; head < h; ++head) {
        const Vec16<bf16_t> q = ld16(rec + head * DH), kv = ld16(rec + (int64_t)kc * ld + dm + head * DH);
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) s = fmaf(q.get(t), kv.get(t), s);
        s = ro_group_sum<HI>(s);
        acc += __expf(s * scale - lse[((int64_t)b * h + head) * N]);
    }
    if (g == 0 && k < N) c[(int64_t)b * N + k] = k < n ? (acc / (float)h + (k == 0 ? 1.f : 0.f)) * 0.5f : 0.f;
}

// the same from the materialised f32 probabilities: one thread per (record, key)
__global__ __launch_bounds__(256) void rollout_cls_f32_kernel(const float *__restrict__ probs, float *__restrict__ c,
                                                              const int32_t *__restrict__ n_tok, int N, int h, int nchunk) {
    const int b = blockIdx.x / nchunk, k = (blockIdx.x - b * nchunk) * 256 + (int)threadIdx.x;
    if (k >= N) return;
    const int n = ro_tokens(n_tok, b, N);
    float v = 0.f;
    if (k < n) {
        float acc = 0.f;
        for (int head = 0; head < h; ++head) acc += probs[((int64_t)b * h + head) * N * N + k];
        v = (acc / (float)h + (k == 0 ? 1.f : 0.f)) * 0.5f;
    }
    c[(int64_t)b * N + k] = v;
}

// =====================================================================================================
// part[b,head,k] = sum_{q < n_b} w[b,q] P[b,head,q,k], bf16: one 4-wave workgroup per (record, head, 128-key block), key on the lane (the K rows
// of the wave's 32 keys stay in registers as the MFMA B operand), loop over 64-query tiles of Q staged in LDS as two 32-row images per 64
// dims -- the loop of the dK / dV kernel of attn_varlen_kernels.h with the dV product replaced by a w-weighted sum over the accumulator rows.
// S = Q K^T by bf16 MFMA (f32 accumulate); p = exp2(s c - lse log2e), acc += w p in f32.  The next tile's rows, lse and w are fetched into
// registers before the MFMAs of the current one and written to LDS behind them.
// Budget: <= 128 VGPRs, no scratch; LDS 8 KiB x HI + 512 B static.
// =====================================================================================================
template <int HI>
__global__ __launch_bounds__(256) void rollout_colsum_kernel(const bf16_t *__restrict__ qkv, const float *__restrict__ lse,
                                                             const float *__restrict__ w, float *__restrict__ part,
                                                             const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off, int N, int h,
                                                             float scale) {
    constexpr int DH = 64 * HI, QB = RO_QT * 128;   // bytes of one Q image
    __shared__ __attribute__((aligned(16))) char smem[HI * QB + 2 * RO_QT * 4];
    char *const Qimg = smem;   // image i at + i QB
    float *const lse_s = reinterpret_cast<float *>(smem + HI * QB), *const w_s = lse_s + RO_QT;
    const int nkb = (N + 127) >> 7;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / h, hd = bh - b * h;
    const int n = ro_tokens(n_tok, b, N);
    if (kb * 128 >= n) return;   // every key of the block is padding (packed: does not exist); the second stage reads keys < n only
    const int d = h * DH;
    const int64_t d3 = 3 * (int64_t)d;
    const bf16_t *base = qkv + ro_row0(tok_off, b, N) * d3 + hd * DH;
    const float *lrow = lse + (int64_t)bh * N, *wrow = w + (int64_t)b * N;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int mykey = kb * 128 + wave * 32 + lr, kc = mykey < n ? mykey : n - 1;   // (keys >= n: clamped loads, nothing stored)
    bf16x8 kf[4 * HI];
#pragma unroll
    for (int ks = 0; ks < 4 * HI; ++ks) kf[ks] = *reinterpret_cast<const bf16x8 *>(base + d + (int64_t)kc * d3 + ks * 16 + 8 * lh);
    const float c = scale * RO_LOG2E;
    const RowOff ro = make_row_off(lane);
    // staging: thread t owns chunk (t & 7) of rows (t >> 3) and (t >> 3) + 32 of every image; threads 0..63 the lse, 64..127 the w of a row
    const int prow = threadIdx.x >> 3, pch = threadIdx.x & 7;
    const int poff0 = img_off(prow, pch * 16), poff1 = img_off(prow + 32, pch * 16);
    u32x4 pre[2 * HI];
    float pside = 0.f;
    auto fetch = [&](int q0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = q0 + prow + 32 * p;
#pragma unroll
            for (int i = 0; i < HI; ++i) {
                u32x4 v = {0u, 0u, 0u, 0u};   // rows >= n: zeros
                if (r < n) v = *reinterpret_cast<const u32x4 *>(base + (int64_t)r * d3 + 64 * i + pch * 8);
                pre[2 * i + p] = v;
            }
        }
        if (threadIdx.x < 2 * RO_QT) {
            const int r = q0 + (int)(threadIdx.x & (RO_QT - 1));
            pside = 0.f;   // rows >= n: lse 0, weight 0 -> p = 1, w p = 0
            if (r < n) pside = threadIdx.x < RO_QT ? lrow[r] * RO_LOG2E : wrow[r];
        }
    };
    float acc = 0.f;
    fetch(0);
    for (int q0 = 0; q0 < n; q0 += RO_QT) {
        __syncthreads();   // everyone is done with the previous tile
#pragma unroll
        for (int i = 0; i < HI; ++i) {
            *reinterpret_cast<u32x4 *>(Qimg + i * QB + poff0) = pre[2 * i];
            *reinterpret_cast<u32x4 *>(Qimg + i * QB + poff1) = pre[2 * i + 1];
        }
        if (threadIdx.x < 2 * RO_QT) lse_s[threadIdx.x] = pside;   // (w_s = lse_s + RO_QT)
        __syncthreads();
        if (q0 + RO_QT < n) fetch(q0 + RO_QT);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (q0 + 32 * t >= n) break;   // (workgroup-uniform)
            // S = Q K^T with the key on the lane; rows = queries q0 + 32 t + 8 (r >> 2) + 4 lh + (r & 3)
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int i = 0; i < HI; ++i)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Qimg + i * QB + t * 4096, ro.ks[ks]), kf[4 * i + ks], s, 0, 0, 0);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 l4 = *reinterpret_cast<const f32x4 *>(&lse_s[32 * t + 8 * g4 + 4 * lh]);
                const f32x4 w4 = *reinterpret_cast<const f32x4 *>(&w_s[32 * t + 8 * g4 + 4 * lh]);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = fmaf(w4[k], __builtin_amdgcn_exp2f(fmaf(s[4 * g4 + k], c, -l4[k])), acc);
            }
        }
    }
    acc += __shfl_xor(acc, 32, 64);   // the two lane halves hold the two halves of every 8-row group
    if (lh == 0 && mykey < n) part[(int64_t)bh * N + mykey] = acc;
}

// the same from the materialised f32 probabilities: one workgroup per (record, head, 64 keys), 64 keys x 4 row slots; slot s adds rows s, s + 4,
// ... in rising order (four loads in flight), the four slot sums meet in LDS and are added in slot order.  HBM-bound: every valid row read once.
__global__ __launch_bounds__(256) void rollout_colsum_f32_kernel(const float *__restrict__ probs, const float *__restrict__ w,
                                                                 float *__restrict__ part, const int32_t *__restrict__ n_tok, int N, int h,
                                                                 int nchunk) {
    __shared__ float red[4][64];
    const int bh = blockIdx.x / nchunk, k = (blockIdx.x - bh * nchunk) * 64 + (int)(threadIdx.x & 63);
    const int b = bh / h, slot = threadIdx.x >> 6;
    const int n = ro_tokens(n_tok, b, N);
    float acc = 0.f;
    if (k < n) {
        const float *p = probs + (int64_t)bh * N * N + k, *wr = w + (int64_t)b * N;
        int q = slot;
        for (; q + 12 < n; q += 16) {
            const float v0 = p[(int64_t)q * N], v1 = p[(int64_t)(q + 4) * N], v2 = p[(int64_t)(q + 8) * N], v3 = p[(int64_t)(q + 12) * N];
            acc = fmaf(wr[q + 12], v3, fmaf(wr[q + 8], v2, fmaf(wr[q + 4], v1, fmaf(wr[q], v0, acc))));
        }
        for (; q < n; q += 4) acc = fmaf(wr[q], p[(int64_t)q * N], acc);
    }
    red[slot][threadIdx.x & 63] = acc;
    __syncthreads();
    if (slot == 0 && k < n) part[(int64_t)bh * N + k] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// second stage of both: r[b,k] = (mean over the heads, in head order, of part[b,head,k] + w[b,k]) / 2; 0 at k >= n_b
__global__ __launch_bounds__(256) void rollout_heads_kernel(const float *__restrict__ part, const float *__restrict__ w, float *__restrict__ r,
                                                            const int32_t *__restrict__ n_tok, int N, int h, int nchunk) {
    const int b = blockIdx.x / nchunk, k = (blockIdx.x - b * nchunk) * 256 + (int)threadIdx.x;
    if (k >= N) return;
    float v = 0.f;
    if (k < ro_tokens(n_tok, b, N)) {
        float s = 0.f;
        for (int head = 0; head < h; ++head) s += part[((int64_t)b * h + head) * N + k];
        v = (s / (float)h + w[(int64_t)b * N + k]) * 0.5f;
    }
    r[(int64_t)b * N + k] = v;
}

// maps[b] /= the maximum over its layers x (n_b - 1) entries (one workgroup per record; IEEE division: the maximum becomes exactly 1)
__global__ __launch_bounds__(256) void rollout_finish_kernel(float *__restrict__ maps, const int32_t *__restrict__ n_tok, int layers, int N) {
    __shared__ float red[4];
    const int b = blockIdx.x, m = ro_tokens(n_tok, b, N) - 1, W = N - 1;
    if (m <= 0) return;   // a record of one token: an empty map, left as it is
    float *rec = maps + (int64_t)b * layers * W;
    float mx = 0.f;
    for (int i = 0; i < layers; ++i)
        for (int j = threadIdx.x; j < m; j += 256) mx = fmaxf(mx, rec[(int64_t)i * W + j]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (!(mx > 0.f)) return;
    for (int i = 0; i < layers; ++i)
        for (int j = threadIdx.x; j < m; j += 256) rec[(int64_t)i * W + j] = __fdiv_rn(rec[(int64_t)i * W + j], mx);
}

bool ro_aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// what both entry points check before anything launches; bf16: P from qkv / lse (probs NULL), f32: P = probs (qkv / lse / tok_off NULL)
bool rollout_args_ok(const void *qkv, const float *lse, const float *probs, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h,
                     int dh, int dtype) {
    if (B <= 0 || N <= 0 || h <= 0 || dh <= 0 || (tok_off && !n_tok)) return false;
    if ((int64_t)B * h * ((N + 63) / 64) >= (1ll << 31) || (int64_t)B * ((N + 15) / 16) >= (1ll << 31)) return false;   // the largest grids of the family
    if (dtype == ECGVIT_BF16)
        return qkv && lse && !probs && (dh == 64 || dh == 128) && N <= ECGVIT_ATTN_MAX_N && ro_aligned16(qkv);
    if (dtype == ECGVIT_F32) return probs && !qkv && !lse && !tok_off;
    return false;
}

}  // namespace

extern "C" {

int64_t ecgvit_rollout_workspace(int B, int N, int h) {
    if (B <= 0 || N <= 0 || h <= 0) return 0;
    return 4ll * B * h * N;
}

int ecgvit_rollout_cls(const void *qkv, const float *lse, const float *probs, float *c, const int32_t *n_tok, const int32_t *tok_off, int B, int N,
                       int h, int dh, float scale, int dtype, void *stream) {
    if (!c || !rollout_args_ok(qkv, lse, probs, n_tok, tok_off, B, N, h, dh, dtype)) return ECGVIT_EINVAL;
    if (dtype == ECGVIT_F32) {
        const int nchunk = (N + 255) / 256;
        hipLaunchKernelGGL(rollout_cls_f32_kernel, dim3((unsigned)(B * nchunk)), dim3(256), 0, as_stream(stream), probs, c, n_tok, N, h, nchunk);
    } else if (dh == 64) {
        const int nchunk = (N + 31) / 32;
        hipLaunchKernelGGL(rollout_cls_kernel<1>, dim3((unsigned)(B * nchunk)), dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, lse, c, n_tok,
                           tok_off, N, h, scale, nchunk);
    } else {
        const int nchunk = (N + 15) / 16;
        hipLaunchKernelGGL(rollout_cls_kernel<2>, dim3((unsigned)(B * nchunk)), dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, lse, c, n_tok,
                           tok_off, N, h, scale, nchunk);
    }
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_rollout_colsum(const void *qkv, const float *lse, const float *probs, const float *w, float *r, void *workspace, const int32_t *n_tok,
                          const int32_t *tok_off, int B, int N, int h, int dh, float scale, int dtype, void *stream) {
    if (!w || !r || !workspace || !rollout_args_ok(qkv, lse, probs, n_tok, tok_off, B, N, h, dh, dtype)) return ECGVIT_EINVAL;
    float *part = (float *)workspace;
    if (dtype == ECGVIT_F32) {
        const int nchunk = (N + 63) / 64;
        hipLaunchKernelGGL(rollout_colsum_f32_kernel, dim3((unsigned)(B * h * nchunk)), dim3(256), 0, as_stream(stream), probs, w, part, n_tok, N, h,
                           nchunk);
    } else {
        const dim3 grid((unsigned)(B * h * ((N + 127) / 128)));
        if (dh == 64)
            hipLaunchKernelGGL(rollout_colsum_kernel<1>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, lse, w, part, n_tok, tok_off, N, h,
                               scale);
        else
            hipLaunchKernelGGL(rollout_colsum_kernel<2>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, lse, w, part, n_tok, tok_off, N, h,
                               scale);
    }
    ECGVIT_CHECK_LAUNCH();
    const int nchunk = (N + 255) / 256;
    hipLaunchKernelGGL(rollout_heads_kernel, dim3((unsigned)(B * nchunk)), dim3(256), 0, as_stream(stream), part, w, r, n_tok, N, h, nchunk);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_rollout_finish(float *maps, const int32_t *n_tok, int B, int layers, int N, void *stream) {
    if (!maps || B <= 0 || layers <= 0 || N <= 0) return ECGVIT_EINVAL;
    if (N == 1) return ECGVIT_OK;   // no patch column
    hipLaunchKernelGGL(rollout_finish_kernel, dim3((unsigned)B), dim3(256), 0, as_stream(stream), maps, n_tok, layers, N);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

}  // extern "C"
