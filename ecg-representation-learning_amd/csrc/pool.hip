// Record pooling: one f32 vector per record from its token rows (the CLS row or the mean over the record's own rows), optionally through the
// classifier's LayerNorm.  HBM-bound: every valid row is read once, 16 B per lane; nothing past a record's n_tok rows is touched.
#include "common.h"

// =====================================================================================================
// One workgroup per (record, column chunk), the chunks of a record adjacent in the grid.  A chunk is 8 lanes x 16 B = 128 B of a row (64 bf16
// / 32 f32 columns): the 512 threads of a workgroup are 64 row slots x 8 lanes, slot s sums rows s, s + 64, s + 128, ... of the record in
// rising order, the 64 slot sums meet in LDS and are added in slot order by one thread per column.  The order of every column's sum is a
// function of the record's own row count alone: the result does not depend on B, on the other records, on where the record's rows start, or
// on N.  Splitting d rather than the rows needs no workspace and no second stage for the sum, and fills the device in both regimes: 512 x 12
// chunks of 251 rows (base) and 16 x 16 chunks of 2049 rows (d = 1024: one workgroup per CU, 4 independent 16-B loads in flight per lane).
// =====================================================================================================
#define POOL_SLOTS 64
#define POOL_THREADS (8 * POOL_SLOTS)

template <typename T>
__global__ __launch_bounds__(POOL_THREADS) void pool_records_kernel(const T *__restrict__ x, float *__restrict__ out,
                                                                    const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off,
                                                                    int N, int d, int mode, int nchunk) {
    constexpr int VN = Vec16<T>::N, CW = 8 * VN;
    __shared__ float part[POOL_SLOTS][CW + 1];
    const int b = blockIdx.x / nchunk, c0 = (blockIdx.x % nchunk) * CW;
    const int sub = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int col = c0 + sub * VN;
    const int n = mode == ECGVIT_POOL_CLS ? 1 : (n_tok ? n_tok[b] : N);
    const int64_t row0 = tok_off ? (int64_t)tok_off[b] : (int64_t)b * N;
    float acc[VN];
#pragma unroll
    for (int k = 0; k < VN; ++k) acc[k] = 0.f;
    if (col < d) {
        const T *p = x + row0 * d + col;
        int r = slot;
        for (; r + 3 * POOL_SLOTS < n; r += 4 * POOL_SLOTS) {   // four independent loads in flight, added in row order
            const Vec16<T> v0 = ld16(p + (int64_t)r * d), v1 = ld16(p + (int64_t)(r + POOL_SLOTS) * d);
            const Vec16<T> v2 = ld16(p + (int64_t)(r + 2 * POOL_SLOTS) * d), v3 = ld16(p + (int64_t)(r + 3 * POOL_SLOTS) * d);
#pragma unroll
            for (int k = 0; k < VN; ++k) acc[k] = (((acc[k] + v0.get(k)) + v1.get(k)) + v2.get(k)) + v3.get(k);
        }
        for (; r < n; r += POOL_SLOTS) {
            const Vec16<T> v = ld16(p + (int64_t)r * d);
#pragma unroll
            for (int k = 0; k < VN; ++k) acc[k] += v.get(k);
        }
    }
#pragma unroll
    for (int k = 0; k < VN; ++k) part[slot][sub * VN + k] = acc[k];
    __syncthreads();
    const int c = threadIdx.x;
    if (c < CW && c0 + c < d) {
        float s = part[0][c];
#pragma unroll 8
        for (int i = 1; i < POOL_SLOTS; ++i) s += part[i][c];
        out[(int64_t)b * d + c0 + c] = s / (float)n;
    }
}

// LayerNorm of the pooled vectors in place (f32 [B, d], biased variance, two passes over registers): one workgroup per record, d <= 2048
__global__ __launch_bounds__(256) void pool_layernorm_kernel(float *__restrict__ out, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, int d, float eps) {
    __shared__ float red[4];
    float *row = out + (int64_t)blockIdx.x * d;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 256 + threadIdx.x;
        v[i] = c < d ? row[c] : 0.f;
        s += v[i];
    }
    const float inv_d = 1.0f / (float)d;
    const float mu = block_sum<4>(s, red) * inv_d;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 256 + threadIdx.x;
        const float t = c < d ? v[i] - mu : 0.f;
        q += t * t;
    }
    const float rs = 1.0f / sqrtf(block_sum<4>(q, red) * inv_d + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = i * 256 + threadIdx.x;
        if (c < d) row[c] = (v[i] - mu) * rs * gamma[c] + beta[c];
    }
}

int ecgvit_pool_records(const void *x, float *out, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int d, int mode,
                        const float *gamma, const float *beta, float eps, int dtype, void *stream) {
    if (!x || !out || B <= 0 || N <= 0 || d <= 0 || d % 8 != 0 || d > ECGVIT_ROW_MAX_D) return ECGVIT_EINVAL;
    if (mode != ECGVIT_POOL_CLS && mode != ECGVIT_POOL_MEAN) return ECGVIT_EINVAL;
    if ((gamma == nullptr) != (beta == nullptr)) return ECGVIT_EINVAL;
    const int rc = dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        constexpr int CW = 8 * Vec16<T>::N;   // the kernel's column chunk
        const int nchunk = (d + CW - 1) / CW;
        if ((int64_t)B * nchunk > 0x7fffffffll) return ECGVIT_EINVAL;
        hipLaunchKernelGGL(pool_records_kernel<T>, dim3(B * nchunk), dim3(POOL_THREADS), 0, as_stream(stream), (const T *)x, out, n_tok, tok_off, N, d,
                           mode, nchunk);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
    if (rc != ECGVIT_OK) return rc;
    if (gamma) {
        hipLaunchKernelGGL(pool_layernorm_kernel, dim3(B), dim3(256), 0, as_stream(stream), out, gamma, beta, d, eps);
        ECGVIT_CHECK_LAUNCH();
    }
    return ECGVIT_OK;
}
