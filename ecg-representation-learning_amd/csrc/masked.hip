// Masked pre-train objective pieces (SimMIM-style; the build's own definition -- the reference has no masked
// objective): mask-token substitution + positional add, row gather / scatter by host-generated
// int32 indices (bit-exact integer indexing), L1 reconstruction loss, and the embedding pair for records of unequal length (packed or
// padded rows).  All HBM-bound, 16 B per lane.
#include "common.h"

namespace {

// one 16-B vector of X: X[row] = (flag[row] ? mask_token : tok[row]) + pos[1 + p], p = the row's patch index inside its record; `flag` marks
// the masked rows, one byte each.  pad: a row past its record's patches (padded layout), written as exact zeros, nothing read
template <typename T>
__device__ __forceinline__ void mask_embed_vec(const T *__restrict__ tok, const float *__restrict__ mask_token, const float *__restrict__ pos,
                                               const uint8_t *__restrict__ flag, T *__restrict__ X, int64_t row, int p, bool pad, int c0, int d) {
    constexpr int VN = Vec16<T>::N;
    Vec16<T> o;
    if (pad) {
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, 0.f);
    } else if (flag[row]) {
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, mask_token[c0 + k] + pos[(int64_t)(1 + p) * d + c0 + k]);
    } else {
        const Vec16<T> v = ld16(tok + row * d + c0);
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, v.get(k) + pos[(int64_t)(1 + p) * d + c0 + k]);
    }
    st16(X + row * d + c0, o);
}

// uniform form (n patches per record, row b * n + p): one flat grid-stride walk over the vectors of X
template <typename T>
__global__ __launch_bounds__(256) void mask_embed_kernel(const T *__restrict__ tok, const float *__restrict__ mask_token,
                                                         const float *__restrict__ pos, const uint8_t *__restrict__ flag,
                                                         T *__restrict__ X, int64_t rows, int n, int d) {
    constexpr int VN = Vec16<T>::N;
    const int dv = d / VN;
    const int64_t total = rows * dv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / dv;
        mask_embed_vec(tok, mask_token, pos, flag, X, row, (int)(row % n), false, (int)(i - row * dv) * VN, d);
    }
}

// ---- table form: records of unequal length (no CLS row).  Record b holds n_tok[b] patches in the rows tok_off[b] .. tok_off[b] + n_tok[b] - 1 of
// tok / X / dX: packed (n_pad == 0: tok_off = exclusive prefix sum of n_tok, no other row exists) or padded (n_pad > 0: tok_off[b] = b * n_pad,
// the rows past n_tok[b] of a record are written as exact zeros and never read).  One grid row per record, its patches strided over the blocks.
template <typename T>
__global__ __launch_bounds__(256) void mask_embed_varlen_kernel(const T *__restrict__ tok, const float *__restrict__ mask_token,
                                                                const float *__restrict__ pos, const uint8_t *__restrict__ flag,
                                                                T *__restrict__ X, const int32_t *__restrict__ n_tok,
                                                                const int32_t *__restrict__ tok_off, int n_pad, int d) {
    constexpr int VN = Vec16<T>::N;
    const int b = blockIdx.y, dv = d / VN;
    const int nb = n_tok[b];
    const int64_t r0 = tok_off[b], total = (int64_t)(n_pad ? n_pad : nb) * dv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int j = (int)(i / dv), c0 = (int)(i - (int64_t)j * dv) * VN;
        mask_embed_vec(tok, mask_token, pos, flag, X, r0 + j, j, j >= nb, c0, d);
    }
}

// backward of mask_embed: dtok = dX where NOT masked (else 0); dmasked = dX where masked (else 0) -> its column sum is the
// mask-token gradient; dpos[1 + p] = sum_b dX[row of (b, p)]   (dpos row 0 = CLS slot, untouched by the masked trunk: zeroed)
// One workgroup per (patch p, group of 8 column vectors): its 256 threads are 8 column vectors x 32 batch lanes, so a wave instruction moves
// 8 records' 128-B segments and n * d / 64 workgroups share the three streams (round 5; the first form -- one THREAD per (p, column vector)
// walking all B records, 94 workgroups at base -- ran at a third of the HBM rate: 313 us for 0.6 GB).  The batch sum is folded over the 32
// lanes through LDS in a fixed order: deterministic.
// One body, forms by template: the lanes walk contributor i = lane, lane + 32, ... of cnt.  The uniform form has cnt = B, contributor i =
// record i, row i * n + p.  TABLES: `order` lists the records by falling n_tok (ties by record index: a fixed order), so the records that hold
// patch p are order[0 .. cnt) with cnt found by bisection -- a workgroup of a tail position touches its few contributors and never walks the
// B records to find them; padded layout (n_pad != 0): the rows (b, p) with p >= n_tok[b] get zeros in dtok / dmasked.
template <typename T, bool TABLES>
__device__ __forceinline__ void mask_embed_bwd_body(const T *__restrict__ dX, const uint8_t *__restrict__ flag, T *__restrict__ dtok,
                                                    T *__restrict__ dmasked, float *__restrict__ dpos, const int32_t *__restrict__ n_tok,
                                                    const int32_t *__restrict__ tok_off, const int32_t *__restrict__ order, int B, int n, int n_pad,
                                                    int d) {
    constexpr int VN = Vec16<T>::N;
    __shared__ float red[32][8][VN];
    const int dv = d / VN, ngrp = (dv + 7) / 8;
    const int p = blockIdx.x / ngrp, cg = blockIdx.x - p * ngrp;
    const int cv = threadIdx.x & 7, bl = threadIdx.x >> 3;
    const int c0 = (cg * 8 + cv) * VN;
    const bool live = cg * 8 + cv < dv;
    int cnt = B;
    if (TABLES) {
        int hi = B;
        cnt = 0;
        while (cnt < hi) {   // first position of `order` whose record is too short for patch p
            const int mid = (cnt + hi) >> 1;
            if (n_tok[order[mid]] > p) cnt = mid + 1;
            else hi = mid;
        }
    }
    float acc[VN];
#pragma unroll
    for (int k = 0; k < VN; ++k) acc[k] = 0.f;
    Vec16<T> zero;
#pragma unroll
    for (int k = 0; k < VN; ++k) zero.set(k, 0.f);
    if (live) {
        for (int i = bl; i < cnt; i += 32) {
            const int64_t row = (TABLES ? (int64_t)tok_off[order[i]] : (int64_t)i * n) + p;
            const Vec16<T> v = ld16(dX + row * d + c0);
#pragma unroll
            for (int k = 0; k < VN; ++k) acc[k] += v.get(k);
            const bool mk = flag[row] != 0;
            st16(dtok + row * d + c0, mk ? zero : v);
            st16(dmasked + row * d + c0, mk ? v : zero);
        }
        if (TABLES && n_pad) {
            for (int i = cnt + bl; i < B; i += 32) {
                const int64_t row = (int64_t)tok_off[order[i]] + p;
                st16(dtok + row * d + c0, zero);
                st16(dmasked + row * d + c0, zero);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VN; ++k) red[bl][cv][k] = acc[k];
    __syncthreads();
    if (bl == 0 && live) {
#pragma unroll
        for (int k = 0; k < VN; ++k) {
            float s = 0.f;
            for (int j = 0; j < 32; ++j) s += red[j][cv][k];
            dpos[(int64_t)(1 + p) * d + c0 + k] = s;
            if (p == 0) dpos[c0 + k] = 0.f;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void mask_embed_bwd_kernel(const T *__restrict__ dX, const uint8_t *__restrict__ flag,
                                                             T *__restrict__ dtok, T *__restrict__ dmasked,
                                                             float *__restrict__ dpos, int B, int n, int d) {
    mask_embed_bwd_body<T, false>(dX, flag, dtok, dmasked, dpos, nullptr, nullptr, nullptr, B, n, 0, d);
}

template <typename T>
__global__ __launch_bounds__(256) void mask_embed_varlen_bwd_kernel(const T *__restrict__ dX, const uint8_t *__restrict__ flag,
                                                                    T *__restrict__ dtok, T *__restrict__ dmasked, float *__restrict__ dpos,
                                                                    const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off,
                                                                    const int32_t *__restrict__ order, int B, int n_pad, int d) {
    mask_embed_bwd_body<T, true>(dX, flag, dtok, dmasked, dpos, n_tok, tok_off, order, B, 0, n_pad, d);
}

// flag[b * nrow + idx[b * m + k]] = 1 for the m indices of each of nb batches (the indexing of rows_by_index_kernel); an index outside
// [0, nrow) is ignored.  (B, n, m) marks the patches of a uniform batch, (1, M, m_total) rows of the whole buffer.
__global__ __launch_bounds__(256) void mark_rows_kernel(const int32_t *__restrict__ idx, uint8_t *__restrict__ flag, int nb, int64_t nrow, int m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nb * m) return;
    const int64_t r = idx[i];
    if (r >= 0 && r < nrow) flag[(i / m) * nrow + r] = 1;
}

// GATHER: out[b*m + k] = in[b*n + idx[b,k]] ; SCATTER: out[b*n + idx[b,k]] = in[b*m + k]
template <typename T, bool SCATTER>
__global__ __launch_bounds__(256) void rows_by_index_kernel(const T *__restrict__ in, const int32_t *__restrict__ idx,
                                                            T *__restrict__ out, int B, int n, int m, int width, int64_t ld_in,
                                                            int64_t ld_out) {
    constexpr int VN = Vec16<T>::N;
    const int wv = width / VN;
    const int64_t total = (int64_t)B * m * wv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / wv;
        const int c0 = (int)(i - r * wv) * VN;
        const int64_t b = r / m;
        const int64_t src = b * n + idx[r];
        if (SCATTER) st16(out + src * ld_out + c0, ld16(in + r * ld_in + c0));
        else st16(out + r * ld_out + c0, ld16(in + src * ld_in + c0));
    }
}

// L1 loss + its gradient, two deterministic stages: L1_BLOCKS blocks each own a contiguous run of elements (8 per thread and pass,
// 16-B accesses when the row pitch allows) and leave one partial sum; a single wave then adds the partials in a fixed order.
constexpr int L1_BLOCKS = 1024;
template <typename T>
__global__ __launch_bounds__(256) void l1_loss_kernel(const T *__restrict__ pred, const T *__restrict__ target,
                                                      float *__restrict__ partial, T *__restrict__ dpred,
                                                      const float *__restrict__ gscalar, int64_t rows, int width, int64_t ld) {
    __shared__ float red[4];
    const float up = (gscalar ? gscalar[0] : 1.0f) / (float)(rows * width);
    const int64_t total = rows * width;
    const int64_t per = (total + gridDim.x - 1) / gridDim.x;
    const int64_t lo = blockIdx.x * per, hi = lo + per < total ? lo + per : total;
    float s = 0.f;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const int64_t r = i / width;
        const int c = (int)(i - r * width);
        const float df = to_f32<T>(pred[r * ld + c]) - to_f32<T>(target[r * ld + c]);
        s += fabsf(df);
        if (dpred) dpred[r * ld + c] = from_f32<T>(df > 0.f ? up : (df < 0.f ? -up : 0.f));
    }
    const float tot = block_sum<4>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ __launch_bounds__(64) void l1_finish_kernel(const float *__restrict__ partial, int n, float *__restrict__ loss, float inv_total) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) s += partial[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) loss[0] = s * inv_total;
}

inline int grid_ew(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 4096)); }

}  // namespace

extern "C" {

// flag_ws = the 0 / 1 mask of `rows` rows: cleared, then (nb, nrow, m) marked as mark_rows_kernel reads them
static int mark_flags(void *flag_ws, int64_t rows, const int32_t *idx, int nb, int64_t nrow, int m, hipStream_t s) {
    if (hipMemsetAsync(flag_ws, 0, (size_t)rows, s) != hipSuccess) return ECGVIT_ELAUNCH;
    if (m > 0) {
        hipLaunchKernelGGL(mark_rows_kernel, dim3((nb * m + 255) / 256), dim3(256), 0, s, idx, (uint8_t *)flag_ws, nb, nrow, m);
        ECGVIT_CHECK_LAUNCH();
    }
    return ECGVIT_OK;
}

int ecgvit_mask_embed_finish(const void *tok, const float *mask_token, const float *pos, const int32_t *idx, void *X,
                                void *flag_ws, int B, int n, int m, int d, int dtype, void *stream) {
    if (B <= 0 || n <= 0 || m < 0 || m > n || d <= 0 || d % 8 != 0 || !flag_ws) return ECGVIT_EINVAL;
    hipStream_t s = as_stream(stream);
    const int64_t rows = (int64_t)B * n;
    const int rc = mark_flags(flag_ws, rows, idx, B, n, m, s);
    if (rc != ECGVIT_OK) return rc;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        hipLaunchKernelGGL(mask_embed_kernel<T>, dim3(grid_ew(rows * d / Vec16<T>::N)), dim3(256), 0, s, (const T *)tok, mask_token, pos,
                           (const uint8_t *)flag_ws, (T *)X, rows, n, d);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_mask_embed_bwd(const void *dX, const void *flag_ws, void *dtok, void *dmasked, float *dpos, int B, int n, int d,
                          int dtype, void *stream) {
    if (B <= 0 || n <= 0 || d <= 0 || d % 8 != 0 || !flag_ws) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        const int grid = n * ((d / Vec16<T>::N + 7) / 8);   // one workgroup per (patch, 8 column vectors)
        hipLaunchKernelGGL(mask_embed_bwd_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)dX, (const uint8_t *)flag_ws, (T *)dtok,
                           (T *)dmasked, dpos, B, n, d);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_mask_embed_varlen_fwd(const void *tok, const float *mask_token, const float *pos, const int32_t *row_idx, void *X, void *flag_ws,
                                 const int32_t *n_tok, const int32_t *tok_off, int B, int N, int n_pad, int64_t M, int m_total, int d,
                                 int dtype, void *stream) {
    if (B <= 0 || B > 65535 || N <= 0 || (n_pad != 0 && n_pad < N) || M < N || m_total < 0 || d <= 0 || d % 8 != 0 || !flag_ws || !n_tok ||
        !tok_off || (m_total > 0 && !row_idx) || (n_pad != 0 && M != (int64_t)B * n_pad))
        return ECGVIT_EINVAL;
    hipStream_t s = as_stream(stream);
    const int rc = mark_flags(flag_ws, M, row_idx, 1, M, m_total, s);
    if (rc != ECGVIT_OK) return rc;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        const int64_t per = (int64_t)(n_pad ? n_pad : N) * d / Vec16<T>::N;
        const dim3 grid((unsigned)std::min<int64_t>((per + 255) / 256, 1024), (unsigned)B);
        hipLaunchKernelGGL(mask_embed_varlen_kernel<T>, grid, dim3(256), 0, s, (const T *)tok, mask_token, pos, (const uint8_t *)flag_ws, (T *)X, n_tok,
                           tok_off, n_pad, d);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_mask_embed_varlen_bwd(const void *dX, const void *flag_ws, void *dtok, void *dmasked, float *dpos, const int32_t *n_tok,
                                 const int32_t *tok_off, const int32_t *order, int B, int N, int n_pad, int d, int dtype, void *stream) {
    if (B <= 0 || N <= 0 || (n_pad != 0 && n_pad < N) || d <= 0 || d % 8 != 0 || !flag_ws || !n_tok || !tok_off || !order) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        const int64_t grid = (int64_t)(n_pad ? n_pad : N) * ((d / Vec16<T>::N + 7) / 8);   // one workgroup per (patch, 8 column vectors)
        if (grid >= (1ll << 31)) return ECGVIT_EINVAL;
        hipLaunchKernelGGL(mask_embed_varlen_bwd_kernel<T>, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), (const T *)dX,
                           (const uint8_t *)flag_ws, (T *)dtok, (T *)dmasked, dpos, n_tok, tok_off, order, B, n_pad, d);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

static int rows_by_index(const void *in, const int32_t *idx, void *out, int B, int n, int m, int64_t width, int64_t ld_in,
                         int64_t ld_out, int dtype, void *stream, bool scatter) {
    if (B <= 0 || n <= 0 || m <= 0 || width <= 0 || width % 8 != 0 || ld_in % 8 != 0 || ld_out % 8 != 0) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        const int g = grid_ew((int64_t)B * m * width / Vec16<T>::N);
#define ROWS(S) hipLaunchKernelGGL((rows_by_index_kernel<T, S>), dim3(g), dim3(256), 0, as_stream(stream), (const T *)in, idx, (T *)out, B, n, m, (int)width, ld_in, ld_out)
        if (scatter) ROWS(true); else ROWS(false);
#undef ROWS
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_gather_rows(const void *in, const int32_t *idx, void *out, int B, int n, int m, int64_t width, int64_t ld_in,
                       int64_t ld_out, int dtype, void *stream) {
    return rows_by_index(in, idx, out, B, n, m, width, ld_in, ld_out, dtype, stream, false);
}

int ecgvit_scatter_rows(const void *in, const int32_t *idx, void *out, int B, int n, int m, int64_t width, int64_t ld_in,
                        int64_t ld_out, int dtype, void *stream) {
    return rows_by_index(in, idx, out, B, n, m, width, ld_in, ld_out, dtype, stream, true);
}

int ecgvit_l1_loss_fwd_bwd(const void *pred, const void *target, float *loss, void *dpred, const float *gscalar, float *partial,
                           int64_t rows, int width, int64_t ld, int dtype, void *stream) {
    if (rows <= 0 || width <= 0 || ld < width || !partial) return ECGVIT_EINVAL;
    const int64_t total = rows * width;
    const int nb = (int)std::min<int64_t>(L1_BLOCKS, (total + 2047) / 2048);
    const int rc = dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        hipLaunchKernelGGL(l1_loss_kernel<T>, dim3(nb), dim3(256), 0, as_stream(stream), (const T *)pred, (const T *)target, partial, (T *)dpred, gscalar, rows, width, ld);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
    if (rc != ECGVIT_OK) return rc;
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(64), 0, as_stream(stream), partial, nb, loss, 1.0f / (float)total);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

}  // extern "C"
