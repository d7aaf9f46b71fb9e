// HBM-bound row / elementwise kernels of the ECG-ViT step: patch gather, CLS+pos, LayerNorm fwd/bwd,
// column sums (bias grads), row softmax (f32 parity path).  All are templated on the activation type
// (float = parity path, bf16 = throughput path), move 16 B per lane per access, reduce with wave64
// shuffles (one row per wave), and keep statistics / parameter gradients in f32.
#include "common.h"

namespace {

// =====================================================================================================
// patch gather: out[(b*n+p)*ld + j*C + c] = x[b][c][p*P + j]      (integer indexing, bit-exact)
// One block = PB consecutive patches of one record: C coalesced row segments -> LDS -> PB contiguous rows.
// =====================================================================================================
// XF = fused input transforms of the reference data pipeline (preprocess/transform.py, wired at ptb_dataset.py:132-149), applied
// while the raw record streams through LDS -- no separate pass over the (B, 12, L) tensor:
//   Normalize    (x - mean[c]) * inv_std[c]                       (transform.py:18-35)
//   TimeEndPad   samples >= lb read as 0 (the record is zero-padded to n * P samples)   (:140-154)
//   TimeOut      samples in [t0[b], t0[b] + tlen[b]) are zeroed   (:175-185; train-time augmentation, host-drawn span)
// One body, forms by template.  The form hands in what it knows of its record: xb / lead = the source base and the lead stride, lb = the valid
// samples, nb = the valid patches, rows = the rows to write, row0 = the first output row.  TABLES (records of unequal length) keeps two early
// exits: a block past `rows` returns (packed rows), a block past nb writes exact zeros and never reads x (padded rows).
template <typename T, bool XF, bool TABLES>
__device__ __forceinline__ void patch_gather_body(const float *__restrict__ xb, int64_t lead, int lb, int nb, int rows, T *__restrict__ out,
                                                  int64_t row0, int C, int P, int PB, int64_t ld, const float *__restrict__ mean,
                                                  const float *__restrict__ inv_std, const int *__restrict__ t0, const int *__restrict__ tlen) {
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [C][PB*P+1]
    const int p0 = blockIdx.x * PB;
    if (TABLES && p0 >= rows) return;
    const int np = min(PB, rows - p0), W = np * P, WS = PB * P + 1;
    const int CP = C * P;
    T *ob = out + (row0 + p0) * ld;
    if (TABLES && p0 >= nb) {
        for (int idx = threadIdx.x; idx < np * (int)ld; idx += 256) ob[idx] = from_f32<T>(0.f);
        return;
    }
    // the block's first sample: part of the 64-bit base in the uniform form, of the 32-bit offset inside the record in the table form
    const int s0 = TABLES ? p0 * P : 0;
    if (!TABLES) xb += (int64_t)p0 * P;
    int z0 = 0, z1 = 0;
    if (XF && t0) { z0 = t0[blockIdx.y]; z1 = z0 + tlen[blockIdx.y]; }
    for (int idx = threadIdx.x; idx < C * W; idx += 256) {
        const int c = idx / W, s = idx - c * W;
        float v;
        if (XF) {
            const int pos = p0 * P + s;
            v = 0.f;
            if (pos < lb && !(pos >= z0 && pos < z1)) v = (xb[(int64_t)c * lead + (s0 + s)] - mean[c]) * inv_std[c];
        } else {
            v = xb[(int64_t)c * lead + (s0 + s)];
        }
        tile[c * WS + s] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < np * (int)ld; idx += 256) {
        const int pp = idx / (int)ld, f = idx - pp * (int)ld;
        float v = 0.f;
        if (f < CP) {
            const int j = f / C, c = f - j * C;
            v = tile[c * WS + pp * P + j];
        }
        ob[(int64_t)pp * ld + f] = from_f32<T>(v);
    }
}

// uniform form: every record holds L (XF: L_raw, zero-padded to L) samples per lead and writes its n = L / P rows
template <typename T, bool XF>
__global__ __launch_bounds__(256) void patch_gather_kernel(const float *__restrict__ x, T *__restrict__ out, int C, int L,
                                                           int P, int n, int PB, int64_t ld, int L_raw,
                                                           const float *__restrict__ mean, const float *__restrict__ inv_std,
                                                           const int *__restrict__ t0, const int *__restrict__ tlen) {
    const int b = blockIdx.y, Lsrc = XF ? L_raw : L;
    patch_gather_body<T, XF, false>(x + (int64_t)b * C * Lsrc, Lsrc, L_raw, n, n, out, (int64_t)b * n, C, P, PB, ld, mean, inv_std, t0, tlen);
}

// table form, the transforms PER RECORD for records of unequal raw length (the reference applies them to one record at a time:
// ptb_dataset.py:132-149): record b holds raw_len[b] samples per lead starting at x + src_off[b] (lead c at + c * lead_stride), is
// zero-padded in normalised space to n_patch[b] * P samples, TimeOut zeroes [t0[b], t0[b] + tlen[b]) of the padded record, and its patch
// rows go to out rows row_off[b] ...  Both row layouts: nrows = 0 -- packed rows, record b writes its n_patch[b] rows; nrows > 0 -- padded
// rows, record b writes nrows rows, exact zeros past n_patch[b].  Record starts fall on arbitrary sample offsets, so the loads are scalar
// (consecutive lanes, consecutive samples of one lead: coalesced); the record base is 64-bit, offsets inside a record 32-bit.
template <typename T>
__global__ __launch_bounds__(256) void patch_gather_transform_varlen_kernel(const float *__restrict__ x, T *__restrict__ out,
                                                                            const int64_t *__restrict__ src_off, int64_t lead_stride,
                                                                            const int32_t *__restrict__ raw_len, const int32_t *__restrict__ n_patch,
                                                                            const int32_t *__restrict__ row_off, int nrows, int n_max, int C, int P,
                                                                            int PB, int64_t ld, const float *__restrict__ mean,
                                                                            const float *__restrict__ inv_std, const int32_t *__restrict__ t0,
                                                                            const int32_t *__restrict__ tlen) {
    const int b = blockIdx.y;
    const int nb = min(n_patch[b], nrows > 0 ? nrows : n_max);   // (a table entry past the rows the launch was sized for never writes there)
    patch_gather_body<T, true, true>(x + src_off[b], lead_stride, min(raw_len[b], nb * P), nb, nrows > 0 ? nrows : nb, out, row_off[b],
                                     C, P, PB, ld, mean, inv_std, t0, tlen);
}

// =====================================================================================================
// CLS concat + positional add (+ embedding dropout)
// =====================================================================================================
// one 16-B vector of X: row `row` = token t of its record, columns c0 ...: the CLS row (t == 0) or row tok_row of tok, + pos[t], then the
// dropout multipliers, drawn at the element index row * d + c0 of X
template <typename T>
__device__ __forceinline__ void embed_finish_vec(const T *__restrict__ tok, const float *__restrict__ cls, const float *__restrict__ pos,
                                                 T *__restrict__ X, int64_t tok_row, int t, int64_t row, int c0, int d, uint64_t seed,
                                                 uint32_t thresh, float inv_keep) {
    constexpr int VN = Vec16<T>::N;
    Vec16<T> o;
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, cls[c0 + k] + pos[c0 + k]);
    } else {
        const Vec16<T> v = ld16(tok + tok_row * (int64_t)d + c0);
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, v.get(k) + pos[(int64_t)t * d + c0 + k]);
    }
    if (thresh) {
        float mk[VN];   // d and c0 are multiples of VN: the run starts on an even element
        dropout_maskN<VN, sizeof(T) == 2>(seed, (uint32_t)row * (uint32_t)d + (uint32_t)c0, thresh, inv_keep, mk);
#pragma unroll
        for (int k = 0; k < VN; ++k) o.set(k, o.get(k) * mk[k]);
    }
    st16(X + row * d + c0, o);
}

// uniform form (n + 1 tokens per record): one flat grid-stride walk over the vectors of X
template <typename T>
__global__ __launch_bounds__(256) void embed_finish_kernel(const T *__restrict__ tok, const float *__restrict__ cls,
                                                           const float *__restrict__ pos, T *__restrict__ X, int B, int n,
                                                           int d, uint64_t seed, uint32_t thresh, float inv_keep) {
    constexpr int VN = Vec16<T>::N;
    const int N = n + 1, dv = d / VN;
    const int64_t total = (int64_t)B * N * dv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int cv = (int)(i % dv);
        const int64_t row = i / dv;
        const int t = (int)(row % N);
        const int64_t b = row / N;
        embed_finish_vec(tok, cls, pos, X, b * n + (t - 1), t, row, cv * VN, d, seed, thresh, inv_keep);
    }
}

// table form, a ragged batch (packed rows): record b's tokens are rows tok_off[b] .. tok_off[b] + n_tok[b] - 1 of X and its patch tokens rows
// tok_off[b] - b .. tok_off[b] - b + n_tok[b] - 2 of tok (tok_off[b] = off_b / P + b); N = the widest record's token count.  Embedding
// dropout draws its bits by packed element index.  One grid row per record, its tokens strided over the blocks.
template <typename T>
__global__ __launch_bounds__(256) void embed_finish_ragged_kernel(const T *__restrict__ tok, const float *__restrict__ cls,
                                                                  const float *__restrict__ pos, T *__restrict__ X, const int32_t *__restrict__ n_tok,
                                                                  const int32_t *__restrict__ tok_off, int N, int d, uint64_t seed, uint32_t thresh,
                                                                  float inv_keep) {
    constexpr int VN = Vec16<T>::N;
    const int b = blockIdx.y, dv = d / VN;
    const int nb = min(n_tok[b], N);
    const int64_t r0 = tok_off[b], total = (int64_t)nb * dv;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int t = (int)(i / dv), c0 = (int)(i - (int64_t)t * dv) * VN;
        embed_finish_vec(tok, cls, pos, X, r0 - b - 1 + t, t, r0 + t, c0, d, seed, thresh, inv_keep);
    }
}

// dtok copy + dpos/dcls reductions over the batch.  One block per (token t, group of 8 16-B column chunks): 8 chunk columns x 32 batch
// lanes; every thread walks its batch residue class (b = lane, lane + 32, ...), then a fixed-order LDS tree over the 32 lanes --
// deterministic, and N * d/(8 VN) blocks of 256 threads instead of one sequential 512-deep loop per thread.
// One body, forms by template: record b's tokens are the rows r0 .. of dX and its patch tokens the rows r0 - b .. of dtok.  The uniform form
// has r0 = b * N, N = n + 1 tokens in every record; TABLES (a ragged batch) reads r0 = tok_off[b] and skips the records with t >= n_tok[b], so
// dpos[t] = the sum over the records that hold token t, gathered per position in a fixed order (no atomics, bit-reproducible); dcls = dpos[0].
template <typename T, bool TABLES>
__device__ __forceinline__ void embed_bwd_body(const T *__restrict__ dX, T *__restrict__ dtok, float *__restrict__ dcls, float *__restrict__ dpos,
                                               const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off, int B, int N, int d,
                                               uint64_t seed, uint32_t thresh, float inv_keep) {
    constexpr int VN = Vec16<T>::N;
    __shared__ float red[32][8 * VN + 1];
    const int dv = d / VN, groups = (dv + 7) / 8;
    const int t = blockIdx.x / groups, cg = blockIdx.x - t * groups;
    const int cc = threadIdx.x & 7, bl = threadIdx.x >> 3;       // chunk column within the group, batch lane
    const int chunk = cg * 8 + cc;
    const bool live = chunk < dv;
    const int c0 = chunk * VN;
    float acc[VN];
#pragma unroll
    for (int k = 0; k < VN; ++k) acc[k] = 0.f;
    if (live) {
        for (int b = bl; b < B; b += 32) {
            if (TABLES && t >= n_tok[b]) continue;
            const int64_t r0 = TABLES ? tok_off[b] : (int64_t)b * N, row = r0 + t;
            Vec16<T> v = ld16(dX + row * d + c0);
            if (thresh) {
                float mk[VN];
                dropout_maskN<VN, sizeof(T) == 2>(seed, (uint32_t)row * (uint32_t)d + (uint32_t)c0, thresh, inv_keep, mk);
#pragma unroll
                for (int k = 0; k < VN; ++k) v.set(k, v.get(k) * mk[k]);
            }
#pragma unroll
            for (int k = 0; k < VN; ++k) acc[k] += v.get(k);
            if (t > 0) st16(dtok + (TABLES ? r0 - b - 1 + t : (int64_t)b * (N - 1) + (t - 1)) * d + c0, v);
        }
    }
#pragma unroll
    for (int k = 0; k < VN; ++k) red[bl][cc * VN + k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 8 * VN) {
        const int col = cg * 8 * VN + threadIdx.x;
        if (col < d) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 32; r += 4) {
                s[0] += red[r][threadIdx.x]; s[1] += red[r + 1][threadIdx.x]; s[2] += red[r + 2][threadIdx.x]; s[3] += red[r + 3][threadIdx.x];
            }
            const float tot = (s[0] + s[1]) + (s[2] + s[3]);
            dpos[(int64_t)t * d + col] = tot;
            if (t == 0) dcls[col] = tot;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const T *__restrict__ dX, T *__restrict__ dtok, float *__restrict__ dcls,
                                                        float *__restrict__ dpos, int B, int n, int d, uint64_t seed,
                                                        uint32_t thresh, float inv_keep) {
    embed_bwd_body<T, false>(dX, dtok, dcls, dpos, nullptr, nullptr, B, n + 1, d, seed, thresh, inv_keep);
}

template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_ragged_kernel(const T *__restrict__ dX, T *__restrict__ dtok, float *__restrict__ dcls,
                                                               float *__restrict__ dpos, const int32_t *__restrict__ n_tok,
                                                               const int32_t *__restrict__ tok_off, int B, int d, uint64_t seed, uint32_t thresh,
                                                               float inv_keep) {
    embed_bwd_body<T, true>(dX, dtok, dcls, dpos, n_tok, tok_off, B, 0, d, seed, thresh, inv_keep);
}

// =====================================================================================================
// LayerNorm: one row per wave, row cached in registers (d <= 64 * VN * MAXV)
// =====================================================================================================
// MAXV = ceil(d / (64 * VN)) rounded up to a power of two, chosen at launch (d <= 2048)

template <typename T, int MAXV>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, T *__restrict__ y,
                                                            float *__restrict__ mean, float *__restrict__ rstd, int64_t rows,
                                                            int d, float eps) {
    constexpr int VN = Vec16<T>::N;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4ll + (threadIdx.x >> 6), nw = gridDim.x * 4ll;
    const float inv_d = 1.0f / (float)d;
    for (int64_t r = wave0; r < rows; r += nw) {
        const T *xr = x + r * d;
        Vec16<T> v[MAXV];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VN;
            if (c < d) {
                v[i] = ld16(xr + c);
#pragma unroll
                for (int k = 0; k < VN; ++k) s += v[i].get(k);
            }
        }
        const float mu = wave_sum(s) * inv_d;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VN;
            if (c < d) {
#pragma unroll
                for (int k = 0; k < VN; ++k) { const float t = v[i].get(k) - mu; q += t * t; }
            }
        }
        const float rs = 1.0f / sqrtf(wave_sum(q) * inv_d + eps);
        T *yr = y + r * d;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VN;
            if (c < d) {
                Vec16<T> o;
#pragma unroll
                for (int k = 0; k < VN; ++k) o.set(k, (v[i].get(k) - mu) * rs * gamma[c + k] + beta[c + k]);
                st16(yr + c, o);
            }
        }
        if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
    }
}

// dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma ; per-block partial dgamma/dbeta.
// FUSED extras (what the NEXT backward stage needs from dx, produced while dx is still in registers):
//   dxm = dx * dropout_mask(seed, element)   (gradient entering the preceding `dropout(Linear) + residual` site)
//   column sums of dxm (or of dx when no dropout) = that Linear's bias gradient -> third partial row
template <typename T, int MAXV, bool EXTRA>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T *__restrict__ dy, const T *__restrict__ x,
                                                            const float *__restrict__ gamma, const float *__restrict__ mean,
                                                            const float *__restrict__ rstd, const T *__restrict__ dres,
                                                            T *__restrict__ dx, float *__restrict__ partial, int64_t rows, int d,
                                                            T *__restrict__ dxm, uint64_t seed, uint32_t thresh, float inv_keep, uint32_t mrp) {
    constexpr int VN = Vec16<T>::N;
    constexpr int NP = EXTRA ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4][NP][d]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t wave0 = blockIdx.x * 4ll + w, nw = gridDim.x * 4ll;
    const float inv_d = 1.0f / (float)d;
    float ag[MAXV][VN], ab[MAXV][VN], gm[MAXV][VN], ac[EXTRA ? MAXV : 1][VN];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * VN;
#pragma unroll
        for (int k = 0; k < VN; ++k) {
            ag[i][k] = 0.f; ab[i][k] = 0.f; gm[i][k] = c < d ? gamma[c + k] : 0.f;
            if (EXTRA) ac[i][k] = 0.f;
        }
    }
    for (int64_t r = wave0; r < rows; r += nw) {
        const float mu = mean[r], rs = rstd[r];
        Vec16<T> vd[MAXV];
        float xh[MAXV][VN];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VN;
            if (c < d) {
                vd[i] = ld16(dy + r * d + c);
                const Vec16<T> vx = ld16(x + r * d + c);
#pragma unroll
                for (int k = 0; k < VN; ++k) {
                    xh[i][k] = (vx.get(k) - mu) * rs;
                    const float g = vd[i].get(k) * gm[i][k];
                    s1 += g;
                    s2 += g * xh[i][k];
                }
            }
        }
        const float c1 = wave_sum(s1) * inv_d, c2 = wave_sum(s2) * inv_d;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VN;
            if (c < d) {
                Vec16<T> o;
                Vec16<T> res;
                if (dres) res = ld16(dres + r * d + c);
#pragma unroll
                for (int k = 0; k < VN; ++k) {
                    const float dyv = vd[i].get(k);
                    float v = rs * (dyv * gm[i][k] - c1 - xh[i][k] * c2);
                    if (dres) v += res.get(k);
                    o.set(k, v);
                    ag[i][k] += dyv * xh[i][k];
                    ab[i][k] += dyv;
                }
                st16(dx + r * d + c, o);
                if (EXTRA) {
                    if (thresh) {
                        Vec16<T> om;
                        float mk[VN];
                        dropout_maskN<VN, sizeof(T) == 2>(seed, (uint32_t)r * mrp * (uint32_t)d + (uint32_t)c, thresh, inv_keep, mk);
#pragma unroll
                        for (int k = 0; k < VN; ++k) om.set(k, o.get(k) * mk[k]);
                        st16(dxm + r * d + c, om);
#pragma unroll
                        for (int k = 0; k < VN; ++k) ac[i][k] += om.get(k);
                    } else {
#pragma unroll
                        for (int k = 0; k < VN; ++k) ac[i][k] += o.get(k);   // the value as stored (rounded)
                    }
                }
            }
        }
    }
    // block reduction of the 4 waves' column sums, then one partial row per block: partial[block][NP][d]
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * VN;
        if (c < d) {
#pragma unroll
            for (int k = 0; k < VN; ++k) {
                red[(w * NP + 0) * d + c + k] = ag[i][k];
                red[(w * NP + 1) * d + c + k] = ab[i][k];
                if (EXTRA) red[(w * NP + 2) * d + c + k] = ac[i][k];
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NP * d; c += 256) {
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) s += red[ww * NP * d + c];
        partial[(int64_t)blockIdx.x * NP * d + c] = s;
    }
}

// =====================================================================================================
// bf16 LayerNorm with an EXACT lane mapping (d = 64 * E, E in {4, 8, 12, 16, 24, 32}): every lane owns E = d/64 elements of a
// row as E/8 16-byte chunks plus, when E % 8 == 4, one 8-byte chunk -- for d = 768 that is 16 B (columns 0..511) + 8 B (columns
// 512..767) per lane, no half-idle second vector as in the MAXV = 2 mapping above: 25 % fewer registers in the backward (4 waves
// per SIMD instead of 3 -> more rows in flight) and no masked lanes.
// =====================================================================================================
template <int E> struct LaneRow {
    static constexpr int N16 = E / 8, N8 = (E % 8) / 4;
    // column of element e of this lane
    static __device__ __forceinline__ int col(int e, int lane) { return e < 8 * N16 ? ((e >> 3) * 64 + lane) * 8 + (e & 7) : 512 * N16 + 4 * lane + (e - 8 * N16); }
    static __device__ __forceinline__ void load(const bf16_t *row, int lane, float (&v)[E]) {
#pragma unroll
        for (int i = 0; i < N16; ++i) {
            const Vec16<bf16_t> t = ld16(row + (i * 64 + lane) * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[8 * i + k] = t.get(k);
        }
        if constexpr (N8 == 1) {
            const bf16x4 t = *reinterpret_cast<const bf16x4 *>(row + 512 * N16 + 4 * lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[8 * N16 + k] = (float)t[k];
        }
    }
    static __device__ __forceinline__ void load_f32(const float *row, int lane, float (&v)[E]) {
#pragma unroll
        for (int i = 0; i < N16; ++i) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(row + (i * 64 + lane) * 8), b = *reinterpret_cast<const f32x4 *>(row + (i * 64 + lane) * 8 + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { v[8 * i + k] = a[k]; v[8 * i + 4 + k] = b[k]; }
        }
        if constexpr (N8 == 1) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(row + 512 * N16 + 4 * lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[8 * N16 + k] = a[k];
        }
    }
    static __device__ __forceinline__ void store(bf16_t *row, int lane, const float (&v)[E]) {
#pragma unroll
        for (int i = 0; i < N16; ++i) {
            Vec16<bf16_t> t;
#pragma unroll
            for (int k = 0; k < 8; ++k) t.set(k, v[8 * i + k]);
            st16(row + (i * 64 + lane) * 8, t);
        }
        if constexpr (N8 == 1) {
            bf16x4 t;
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = (bf16_t)v[8 * N16 + k];
            *reinterpret_cast<bf16x4 *>(row + 512 * N16 + 4 * lane) = t;
        }
    }
    // the 8-bit copy of a row: v = the values as stored, inv = q8_inverse(scale); amax = max(amax, max |v|)
    template <int FMT> static __device__ __forceinline__ void store8(uint8_t *row, int lane, const float (&v)[E], float inv, float &amax) {
#pragma unroll
        for (int i = 0; i < N16; ++i)
            *reinterpret_cast<u32x2 *>(row + (i * 64 + lane) * 8) = u32x2{q8_encode4<FMT>(v + 8 * i, inv, amax), q8_encode4<FMT>(v + 8 * i + 4, inv, amax)};
        if constexpr (N8 == 1) *reinterpret_cast<uint32_t *>(row + 512 * N16 + 4 * lane) = q8_encode4<FMT>(v + 8 * N16, inv, amax);
    }
};

// Q8: additionally y8 = the e4m3 copy of y (the operand of the next Linear's fp8 product, written here instead of by a quantise pass
// over y) at *q8_scale, and *q8_amax = max(*q8_amax, max |y|)
template <int E, bool Q8 = false>
__global__ __launch_bounds__(256) void layernorm_fwd_fit_kernel(const bf16_t *__restrict__ x, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, bf16_t *__restrict__ y,
                                                                float *__restrict__ mean, float *__restrict__ rstd, int64_t rows, float eps,
                                                                uint8_t *__restrict__ y8 = nullptr, const float *__restrict__ q8_scale = nullptr,
                                                                float *__restrict__ q8_amax = nullptr) {
    using L = LaneRow<E>;
    [[maybe_unused]] float q8_inv = 0.f, qmax = 0.f;
    if constexpr (Q8) q8_inv = q8_inverse(*q8_scale);
    constexpr int d = 64 * E;
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4ll + (threadIdx.x >> 6), nw = gridDim.x * 4ll;
    float gm[E], bt[E];
    L::load_f32(gamma, lane, gm);
    L::load_f32(beta, lane, bt);
    for (int64_t r = wave0; r < rows; r += nw) {
        float v[E];
        L::load(x + r * d, lane, v);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) s += v[k];
        const float mu = wave_sum(s) * (1.0f / d);
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) { v[k] -= mu; q += v[k] * v[k]; }
        const float rs = 1.0f / sqrtf(wave_sum(q) * (1.0f / d) + eps);
#pragma unroll
        for (int k = 0; k < E; ++k) v[k] = v[k] * rs * gm[k] + bt[k];
        if (!Q8 || y) L::store(y + r * d, lane, v);   // (Q8: y may be NULL -- every consumer reads the 8-bit copy)
        if constexpr (Q8) {
#pragma unroll
            for (int k = 0; k < E; ++k) v[k] = (float)(bf16_t)v[k];   // the value as stored
            L::template store8<ECGVIT_FP8_E4M3>(y8 + r * d, lane, v, q8_inv, qmax);
        }
        if (lane == 0) { mean[r] = mu; rstd[r] = rs; }
    }
    if constexpr (Q8) {
        wave_amax_publish(q8_amax, qmax);
    }
}

// Q8 (with EXTRA): additionally g8 = the e5m2 copy of v = the gradient the next backward stage consumes (dxm when a mask is applied,
// else dx) -- the 8-bit A operand of that stage's input-gradient product, written here instead of by a quantise pass -- at *q8_scale,
// and *q8_amax = max(*q8_amax, max |v|)
template <int E, bool EXTRA, bool Q8 = false>
__global__ __launch_bounds__(256, E <= 12 ? 4 : 2) void layernorm_bwd_fit_kernel(const bf16_t *__restrict__ dy, const bf16_t *__restrict__ x,
                                                                const float *__restrict__ gamma, const float *__restrict__ mean,
                                                                const float *__restrict__ rstd, const bf16_t *__restrict__ dres,
                                                                bf16_t *__restrict__ dx, float *__restrict__ partial, int64_t rows,
                                                                bf16_t *__restrict__ dxm, uint64_t seed, uint32_t thresh, float inv_keep,
                                                                uint8_t *__restrict__ g8 = nullptr, const float *__restrict__ q8_scale = nullptr,
                                                                float *__restrict__ q8_amax = nullptr, uint32_t mrp = 1) {
    using L = LaneRow<E>;
    [[maybe_unused]] float q8_inv = 0.f, qmax = 0.f;
    if constexpr (Q8) q8_inv = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, q8_inverse(*q8_scale))));
    constexpr int d = 64 * E, NP = EXTRA ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) float red[];  // [4][NP][d] partial sums, then gamma [d]
    // (w and the Q8 reciprocal as SCALARS: the row index, its offsets and mean / rstd then live in SGPRs)
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t wave0 = blockIdx.x * 4ll + w, nw = gridDim.x * 4ll;
    float *gs = red + 4 * NP * d;   // gamma lives in LDS (3 reads per row) instead of E registers: the kernel fits 128 VGPRs = 4 waves/SIMD
    for (int c = threadIdx.x; c < d; c += 256) gs[c] = gamma[c];
    __syncthreads();
    float ag[E], ab[E], ac[EXTRA ? E : 1];
#pragma unroll
    for (int k = 0; k < E; ++k) { ag[k] = 0.f; ab[k] = 0.f; if (EXTRA) ac[k] = 0.f; }
    for (int64_t r = wave0; r < rows; r += nw) {
        // the lane index, taken anew per row: hipcc otherwise keeps one 64-bit per-lane pointer per tensor (dy, x, dres, dx, dxm, g8: 12 VGPRs) across
        // the loop instead of one 32-bit offset beside the scalar row bases -- with them the E = 12 and E = 32 forms spilled (tests/test_code_objects.py)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        ln &= 63;
        const float mu = mean[r], rs = rstd[r];
        const uint32_t ro = (uint32_t)r * (uint32_t)d;   // 32-bit element offset (rows * d < 2^31 checked by the launcher): scalar base + one VGPR offset per access
        float g[E], xh[E], gm[E];
        L::load(dy + ro, ln, g);
        L::load(x + ro, ln, xh);
        L::load_f32(gs, ln, gm);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < E; ++k) {
            xh[k] = (xh[k] - mu) * rs;
            ag[k] += g[k] * xh[k];
            ab[k] += g[k];
            g[k] *= gm[k];
            s1 += g[k];
            s2 += g[k] * xh[k];
        }
        const float c1 = wave_sum(s1) * (1.0f / d), c2 = wave_sum(s2) * (1.0f / d);
        float o[E];
        if (dres) L::load(dres + ro, ln, o);
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const float v = rs * (g[k] - c1 - xh[k] * c2);
            o[k] = (float)(bf16_t)(dres ? o[k] + v : v);   // the value as stored (rounded): what dxm and the column sums see
        }
        L::store(dx + ro, ln, o);
        if (EXTRA) {
            if (thresh) {
                const uint32_t mo = ro * mrp;   // mask counter of row r * mrp (ecgvit_layernorm_bwd_fused_rowpitch)
#pragma unroll
                for (int i = 0; i < L::N16; ++i) {
                    float mk[8];
                    dropout_maskN<8, true>(seed, mo + (uint32_t)((i * 64 + ln) * 8), thresh, inv_keep, mk);
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[8 * i + k] = (float)(bf16_t)(o[8 * i + k] * mk[k]);
                }
                if constexpr (L::N8 == 1) {
                    float mk[4];
                    dropout_maskN<4, true>(seed, mo + (uint32_t)(512 * L::N16 + 4 * ln), thresh, inv_keep, mk);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[8 * L::N16 + k] = (float)(bf16_t)(o[8 * L::N16 + k] * mk[k]);
                }
                if (!Q8 || dxm) L::store(dxm + ro, ln, o);   // (Q8: dxm may be NULL -- the masked gradient leaves as g8 only)
            }
#pragma unroll
            for (int k = 0; k < E; ++k) ac[k] += o[k];
            if constexpr (Q8) L::template store8<ECGVIT_BF8_E5M2>(g8 + ro, ln, o, q8_inv, qmax);   // o = the values as stored (bf16-rounded), masked if a mask applies
        }
    }
    if constexpr (Q8) {
        wave_amax_publish(q8_amax, qmax);
    }
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int c = L::col(k, lane);
        red[(w * NP + 0) * d + c] = ag[k];
        red[(w * NP + 1) * d + c] = ab[k];
        if (EXTRA) red[(w * NP + 2) * d + c] = ac[k];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < NP * d; c += 256) {
        float s = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) s += red[ww * NP * d + c];
        partial[(int64_t)blockIdx.x * NP * d + c] = s;
    }
}

// out[c] = sum_p partial[p][c]  for c < width ; optional split into two or three outputs (dgamma | dbeta | dcolsum).
// Block = 64 columns x 16 row slices (each slice sums every 16th partial row, 4 loads in flight), LDS combine.
__global__ __launch_bounds__(1024) void reduce_partials_kernel(const float *__restrict__ partial, int nparts, int width,
                                                               float *__restrict__ out0, float *__restrict__ out1, int split,
                                                               float *__restrict__ out2 = nullptr) {
    // block = 64 columns x 16 row slices (the grid is only width/64 blocks, so the parallelism has to come from inside the block);
    // every slice sums each 16th partial row with 4 loads in flight; fixed-order LDS tree -> deterministic
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < width) {
        int p = slice;
        for (; p + 48 < nparts; p += 64) {
            s0 += partial[(int64_t)p * width + c];
            s1 += partial[(int64_t)(p + 16) * width + c];
            s2 += partial[(int64_t)(p + 32) * width + c];
            s3 += partial[(int64_t)(p + 48) * width + c];
        }
        for (; p < nparts; p += 16) s0 += partial[(int64_t)p * width + c];
    }
    red[slice][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (slice == 0 && c < width) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 4) { t[0] += red[r][lane]; t[1] += red[r + 1][lane]; t[2] += red[r + 2][lane]; t[3] += red[r + 3][lane]; }
        const float s = (t[0] + t[1]) + (t[2] + t[3]);
        if (c < split) out0[c] = s;
        else if (c < 2 * split || !out2) out1[c - split] = s;
        else out2[c - 2 * split] = s;
    }
}

// =====================================================================================================
// column sums: out[n] = sum_m in[m][n]
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T *__restrict__ in, int64_t ld, float *__restrict__ partial, int64_t M,
                                                     int N, int rows_per_block) {
    constexpr int VN = Vec16<T>::N;
    __shared__ float red[4][64 * VN];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * VN;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(M, r0 + rows_per_block);
    float acc[VN];
#pragma unroll
    for (int k = 0; k < VN; ++k) acc[k] = 0.f;
    if (c < N) {
        for (int64_t r = r0 + w; r < r1; r += 4) {
            const Vec16<T> v = ld16(in + r * ld + c);
#pragma unroll
            for (int k = 0; k < VN; ++k) acc[k] += v.get(k);
        }
    }
#pragma unroll
    for (int k = 0; k < VN; ++k) red[w][lane * VN + k] = acc[k];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * VN; i += 256) {
        const int cc = blockIdx.x * 64 * VN + i;
        if (cc < N) partial[(int64_t)blockIdx.y * N + cc] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    }
}

// =====================================================================================================
// f32 parity-path softmax over materialised scores: one row per wave
// =====================================================================================================
__global__ __launch_bounds__(256) void softmax_rows_kernel(float *__restrict__ S, int64_t rows, int N, int64_t ld) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4ll + (threadIdx.x >> 6), nw = gridDim.x * 4ll;
    for (int64_t r = wave0; r < rows; r += nw) {
        float *s = S + r * ld;
        float m = -INFINITY;
        for (int c = lane; c < N; c += 64) m = fmaxf(m, s[c]);
        m = wave_max(m);
        float sum = 0.f;
        for (int c = lane; c < N; c += 64) sum += expf(s[c] - m);
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int c = lane; c < N; c += 64) s[c] = expf(s[c] - m) * inv;
    }
}

__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float *__restrict__ P, float *__restrict__ dP, int64_t rows,
                                                               int N, int64_t ld, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = blockIdx.x * 4ll + (threadIdx.x >> 6), nw = gridDim.x * 4ll;
    for (int64_t r = wave0; r < rows; r += nw) {
        const float *p = P + r * ld;
        float *g = dP + r * ld;
        float dot = 0.f;
        for (int c = lane; c < N; c += 64) dot += p[c] * g[c];
        dot = wave_sum(dot);
        for (int c = lane; c < N; c += 64) g[c] = p[c] * (g[c] - dot) * scale;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void dropout_apply_kernel(const T *__restrict__ in, T *__restrict__ out, int64_t count,
                                                            uint64_t seed, uint32_t thresh, float inv_keep, uint32_t cols, uint32_t mrp) {
    constexpr int VN = Vec16<T>::N;
    const int64_t nv = count / VN;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        Vec16<T> v = ld16(in + i * VN);
        float mk[VN];
        uint32_t idx = (uint32_t)i * (uint32_t)VN;
        if (mrp != 1) idx += idx / cols * (mrp - 1) * cols;   // compact row r draws the mask of row r * mrp (cols % VN == 0)
        dropout_maskN<VN, sizeof(T) == 2>(seed, idx, thresh, inv_keep, mk);
#pragma unroll
        for (int k = 0; k < VN; ++k) v.set(k, v.get(k) * mk[k]);
        st16(out + i * VN, v);
    }
}

inline int grid_for_rows(int64_t rows) { return (int)std::min<int64_t>((rows + 3) / 4, 2048); }

}  // namespace

static bool ln_fit(int d) { const int e = d / 64; return d % 256 == 0 && (e == 4 || e == 8 || e == 12 || e == 16 || e == 24 || e == 32); }   // exact lane mapping available
// the LayerNorm launchers' one routing: f(form), the form a type.  bf16 at an exact width takes LnExact<d / 64>, the exact-lane kernels, where
// `exact_ok` (the caller's statement that their offsets suffice); everything else takes LnMasked<T, MAXV>, the generic kernels, MAXV = the 16-byte
// vectors of a row per lane rounded up to a power of two
template <int E_> struct LnExact { using T = bf16_t; static constexpr bool EXACT = true; static constexpr int E = E_; };
template <typename T_, int MAXV_> struct LnMasked { using T = T_; static constexpr bool EXACT = false; static constexpr int MAXV = MAXV_; };
template <typename F> static int ln_dispatch(int dtype, int d, bool exact_ok, F &&f) {
    if (dtype == ECGVIT_BF16 && exact_ok && ln_fit(d)) switch (d / 64) {
        case 4: return f(LnExact<4>{});    case 8: return f(LnExact<8>{});    case 12: return f(LnExact<12>{});
        case 16: return f(LnExact<16>{});  case 24: return f(LnExact<24>{});  case 32: return f(LnExact<32>{});
    }
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        constexpr int WV = 64 * Vec16<T>::N;   // the elements of a row one vector per lane covers
        const int nv = (d + WV - 1) / WV;
        if (nv <= 1) return f(LnMasked<T, 1>{});
        if (nv <= 2) return f(LnMasked<T, 2>{});
        if (nv <= 4) return f(LnMasked<T, 4>{});
        if constexpr (WV == 256) return f(LnMasked<T, 8>{});   // (d <= 2048: four bf16 vectors per lane always suffice)
        return ECGVIT_EINVAL;
    });
}
// ---------------------------------------------------------------------------------------------------
extern "C" {

// the gather's LDS tile: C * (PB * P + 1) floats, PB patches per block halved until the tile fits 48 KiB; false: one patch alone passes 64 KiB
static bool patch_tile(int C, int P, int &PB, size_t &lds) {
    PB = std::max(1, 256 / P);
    while (PB > 1 && (size_t)C * (PB * P + 1) * 4 > 48 * 1024) PB >>= 1;
    lds = (size_t)C * (PB * P + 1) * 4;
    return lds <= 64 * 1024;
}

static int patch_gather_launch(const float *x, void *patches, int B, int C, int L, int P, int64_t ld, int dtype, void *stream, bool xf,
                               int L_raw, const float *mean, const float *inv_std, const int *t0, const int *tlen) {
    if (B <= 0 || C <= 0 || P <= 0 || L <= 0 || L % P != 0 || ld < (int64_t)C * P) return ECGVIT_EINVAL;
    if (xf && (!mean || !inv_std || L_raw <= 0 || L_raw > L || ((t0 == nullptr) != (tlen == nullptr)))) return ECGVIT_EINVAL;
    const int n = L / P;
    int PB;
    size_t lds;
    if (!patch_tile(C, P, PB, lds)) return ECGVIT_EINVAL;
    dim3 grid((n + PB - 1) / PB, B);
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
#define PG(X) hipLaunchKernelGGL((patch_gather_kernel<T, X>), grid, dim3(256), lds, as_stream(stream), x, (T *)patches, C, L, P, n, PB, ld, L_raw, mean, inv_std, t0, tlen)
        if (xf) PG(true); else PG(false);
#undef PG
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_patch_gather(const float *x, void *patches, int B, int C, int L, int P, int64_t ld, int dtype, void *stream) {
    return patch_gather_launch(x, patches, B, C, L, P, ld, dtype, stream, false, L, nullptr, nullptr, nullptr, nullptr);
}

int ecgvit_patch_gather_transform(const float *x_raw, void *patches, int B, int C, int L_raw, int L, int P, int64_t ld,
                                  const float *mean, const float *inv_std, const int32_t *timeout_start, const int32_t *timeout_len,
                                  int dtype, void *stream) {
    return patch_gather_launch(x_raw, patches, B, C, L, P, ld, dtype, stream, true, L_raw, mean, inv_std, timeout_start, timeout_len);
}

int ecgvit_patch_gather_transform_varlen(const float *x, void *patches, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len,
                                         const int32_t *n_patch, const int32_t *row_off, int n_rows_per_record, int n_max, int B, int C, int P,
                                         int64_t ld, const float *mean, const float *inv_std, const int32_t *timeout_start,
                                         const int32_t *timeout_len, int dtype, void *stream) {
    if (B <= 0 || C <= 0 || P <= 0 || n_max <= 0 || n_rows_per_record < 0 || lead_stride <= 0 || ld < (int64_t)C * P) return ECGVIT_EINVAL;
    if (!x || !patches || !src_off || !raw_len || !n_patch || !row_off || !mean || !inv_std) return ECGVIT_EINVAL;
    if ((timeout_start == nullptr) != (timeout_len == nullptr)) return ECGVIT_EINVAL;
    if (n_rows_per_record > 0 && n_rows_per_record < n_max) return ECGVIT_EINVAL;
    if (B > 65535 || (int64_t)n_max * ld > INT32_MAX) return ECGVIT_EINVAL;   // (grid.y; 32-bit offsets inside a record)
    int PB;
    size_t lds;
    if (!patch_tile(C, P, PB, lds)) return ECGVIT_EINVAL;
    const int rows = n_rows_per_record > 0 ? n_rows_per_record : n_max;
    dim3 grid((rows + PB - 1) / PB, B);
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        hipLaunchKernelGGL(patch_gather_transform_varlen_kernel<T>, grid, dim3(256), lds, as_stream(stream), x, (T *)patches, src_off, lead_stride,
                           raw_len, n_patch, row_off, n_rows_per_record, n_max, C, P, PB, ld, mean, inv_std, timeout_start, timeout_len);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

// the embedding launchers: d a multiple of 8 (a whole 16-B vector of either type); a dropout rate the element type cannot apply is refused
// (bf16: p applied as round(256 p) / 256; below 1/512: rejected)
int ecgvit_embed_finish(const void *tok, const float *cls, const float *pos, void *X, int B, int n, int d, float dropout_p,
                        uint64_t seed, int dtype, void *stream) {
    if (B <= 0 || n <= 0 || d <= 0 || d % 8 != 0) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        uint32_t th;
        float ik;
        if (!dropout_site_params(dropout_p, sizeof(T) == 2, th, ik)) return ECGVIT_EINVAL;
        const int64_t total = (int64_t)B * (n + 1) * d / Vec16<T>::N;
        const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(embed_finish_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)tok, cls, pos, (T *)X, B, n, d, seed, th, ik);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_embed_bwd(const void *dX, void *dtok, float *dcls, float *dpos, int B, int n, int d, float dropout_p, uint64_t seed,
                     int dtype, void *stream) {
    if (B <= 0 || n <= 0 || d <= 0 || d % 8 != 0) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        uint32_t th;
        float ik;
        if (!dropout_site_params(dropout_p, sizeof(T) == 2, th, ik)) return ECGVIT_EINVAL;
        const int grid = (n + 1) * ((d / Vec16<T>::N + 7) / 8);   // one block per (token, group of 8 column chunks)
        hipLaunchKernelGGL(embed_bwd_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)dX, (T *)dtok, dcls, dpos, B, n, d, seed, th, ik);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_embed_finish_ragged(const void *tok, const float *cls, const float *pos, void *X, const int32_t *n_tok, const int32_t *tok_off, int B,
                               int N, int d, float dropout_p, uint64_t seed, int dtype, void *stream) {
    if (B <= 0 || B > 65535 || N <= 0 || d <= 0 || d % 8 != 0 || !n_tok || !tok_off) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        uint32_t th;
        float ik;
        if (!dropout_site_params(dropout_p, sizeof(T) == 2, th, ik)) return ECGVIT_EINVAL;
        const int64_t per = (int64_t)N * d / Vec16<T>::N;
        const dim3 grid((unsigned)std::min<int64_t>((per + 255) / 256, 1024), (unsigned)B);
        hipLaunchKernelGGL(embed_finish_ragged_kernel<T>, grid, dim3(256), 0, as_stream(stream), (const T *)tok, cls, pos, (T *)X, n_tok, tok_off, N, d,
                           seed, th, ik);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_embed_bwd_ragged(const void *dX, void *dtok, float *dcls, float *dpos, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int d,
                            float dropout_p, uint64_t seed, int dtype, void *stream) {
    if (B <= 0 || N <= 0 || d <= 0 || d % 8 != 0 || !n_tok || !tok_off) return ECGVIT_EINVAL;
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        uint32_t th;
        float ik;
        if (!dropout_site_params(dropout_p, sizeof(T) == 2, th, ik)) return ECGVIT_EINVAL;
        const int grid = N * ((d / Vec16<T>::N + 7) / 8);   // one block per (token, group of 8 column chunks)
        hipLaunchKernelGGL(embed_bwd_ragged_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)dX, (T *)dtok, dcls, dpos, n_tok, tok_off,
                           B, d, seed, th, ik);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

// y8: the forward that also emits the 8-bit copy, an exact-lane kernel only (its callers have checked ln_fit(d)).  The forward's row bases are
// 64-bit in either form, so the exact-lane kernels serve any row count
static int ln_fwd_launch(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd, int64_t rows, int d, float eps,
                         int dtype, void *stream, void *y8 = nullptr, const float *q8_scale = nullptr, float *q8_amax = nullptr) {
    const int grid = grid_for_rows(rows);
    return ln_dispatch(dtype, d, true, [&](auto form) -> int {
        using Form = decltype(form);
        using T = typename Form::T;
        if constexpr (Form::EXACT) {
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)x, gamma, beta, (T *)y, mean, rstd, rows, eps, (uint8_t *)y8, q8_scale, q8_amax);
            };
            if (y8) launch(layernorm_fwd_fit_kernel<Form::E, true>); else launch(layernorm_fwd_fit_kernel<Form::E, false>);
        } else {
            if (y8) return ECGVIT_EINVAL;
            hipLaunchKernelGGL((layernorm_fwd_kernel<T, Form::MAXV>), dim3(grid), dim3(256), 0, as_stream(stream), (const T *)x, gamma, beta, (T *)y, mean, rstd, rows, d, eps);
        }
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd, int64_t rows,
                         int d, float eps, int dtype, void *stream) {
    if (rows <= 0 || d <= 0 || d % 8 != 0 || d > ECGVIT_ROW_MAX_D) return ECGVIT_EINVAL;
    return ln_fwd_launch(x, gamma, beta, y, mean, rstd, rows, d, eps, dtype, stream);
}

// bf16 LayerNorm forward that also writes the e4m3 copy of its output (d = 64 * {4, 8, 12, 16, 24, 32} only)
int ecgvit_layernorm_fwd_q8(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd, int64_t rows, int d,
                            float eps, void *y8, const float *q8_scale, float *q8_amax, void *stream) {
    if (rows <= 0 || !ln_fit(d) || !y8 || !q8_scale || !q8_amax) return ECGVIT_EINVAL;
    return ln_fwd_launch(x, gamma, beta, y, mean, rstd, rows, d, eps, ECGVIT_BF16, stream, y8, q8_scale, q8_amax);
}

static int ln_bwd_grid(int64_t rows) { return (int)std::min<int64_t>((rows + 3) / 4, 1024); }  // up to 4 resident blocks per CU (the exact-lane kernels at E <= 12; the others hold fewer)

int64_t ecgvit_layernorm_bwd_workspace(int64_t rows, int d) { return (int64_t)ln_bwd_grid(rows) * 3 * d * 4; }

static int ln_bwd_launch(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                         void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d, int dtype, void *stream,
                         bool extra, void *dxm, float *dcolsum, float dropout_p, uint64_t seed,
                         void *g8 = nullptr, const float *q8_scale = nullptr, float *q8_amax = nullptr, int mask_row_pitch = 1) {
    if (mask_row_pitch < 1 || (mask_row_pitch > 1 && (g8 || rows * mask_row_pitch * d >= (1ll << 32)))) return ECGVIT_EINVAL;
    const uint32_t mrp = (uint32_t)mask_row_pitch;
    if (g8 && (!extra || !q8_scale || !q8_amax || dtype != ECGVIT_BF16 || !ln_fit(d) || (int64_t)rows * d >= (1ll << 31))) return ECGVIT_EINVAL;
    if (rows <= 0 || d <= 0 || d % 8 != 0 || d > ECGVIT_ROW_MAX_D || !partial) return ECGVIT_EINVAL;
    if (extra && (!dcolsum || (dropout_p > 0.f && !dxm && !g8) || ((int64_t)rows * d) % 2)) return ECGVIT_EINVAL;
    const int grid = ln_bwd_grid(rows);
    const int np = extra ? 3 : 2;
    const size_t lds = (size_t)4 * np * d * 4;
    if (dtype != ECGVIT_F32 && dtype != ECGVIT_BF16) return ECGVIT_EINVAL;
    uint32_t th;
    float ik;
    if (!dropout_site_params(dropout_p, dtype == ECGVIT_BF16, th, ik)) return ECGVIT_EINVAL;   // (bf16: p applied as round(256 p) / 256; below 1/512: rejected)
    // the exact-lane kernels' 32-bit element offsets need rows * d < 2^31; past it the generic kernels take over
    const int rc = ln_dispatch(dtype, d, (int64_t)rows * d < (1ll << 31), [&](auto form) -> int {
        using Form = decltype(form);
        using T = typename Form::T;
        if constexpr (Form::EXACT) {
            auto launch = [&](auto kernel) {   // (+ gamma in LDS)
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds + (size_t)d * 4, as_stream(stream), (const T *)dy, (const T *)x, gamma, mean, rstd, (const T *)dres, (T *)dx, (float *)partial, rows, (T *)dxm, seed, th, ik, (uint8_t *)g8, q8_scale, q8_amax, mrp);
            };
            if (g8) launch(layernorm_bwd_fit_kernel<Form::E, true, true>);
            else if (extra) launch(layernorm_bwd_fit_kernel<Form::E, true, false>);
            else launch(layernorm_bwd_fit_kernel<Form::E, false, false>);
        } else {
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, as_stream(stream), (const T *)dy, (const T *)x, gamma, mean, rstd, (const T *)dres, (T *)dx, (float *)partial, rows, d, (T *)dxm, seed, th, ik, mrp);
            };
            if (g8) return ECGVIT_EINVAL;   // (g8 has passed ln_fit(d) and rows * d < 2^31 above: never reached)
            if (extra) launch(layernorm_bwd_kernel<T, Form::MAXV, true>);
            else launch(layernorm_bwd_kernel<T, Form::MAXV, false>);
        }
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
    if (rc != ECGVIT_OK) return rc;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((np * d + 63) / 64), dim3(1024), 0, as_stream(stream), (const float *)partial, grid, np * d, dgamma, dbeta, d, extra ? dcolsum : nullptr);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_layernorm_bwd(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                         void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d, int dtype, void *stream) {
    return ln_bwd_launch(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, partial, rows, d, dtype, stream, false, nullptr, nullptr, 0.f, 0);
}

int ecgvit_layernorm_bwd_fused(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                               void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d, void *dxm, float *dcolsum,
                               float dropout_p, uint64_t seed, int dtype, void *stream) {
    return ln_bwd_launch(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, partial, rows, d, dtype, stream, true, dxm, dcolsum, dropout_p, seed);
}

int ecgvit_layernorm_bwd_fused_rowpitch(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                                        void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d, void *dxm, float *dcolsum,
                                        float dropout_p, uint64_t seed, int mask_row_pitch, int dtype, void *stream) {
    return ln_bwd_launch(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, partial, rows, d, dtype, stream, true, dxm, dcolsum, dropout_p, seed,
                         nullptr, nullptr, nullptr, mask_row_pitch);
}

int ecgvit_layernorm_bwd_fused_q8(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd, const void *dres,
                                  void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d, void *dxm, float *dcolsum,
                                  float dropout_p, uint64_t seed, void *g8, const float *q8_scale, float *q8_amax, void *stream) {
    if (!g8) return ECGVIT_EINVAL;
    return ln_bwd_launch(dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, partial, rows, d, ECGVIT_BF16, stream, true, dxm, dcolsum, dropout_p, seed,
                         g8, q8_scale, q8_amax);
}

static int colsum_row_blocks(int64_t M) { return (int)std::min<int64_t>((M + 255) / 256, 256); }

int64_t ecgvit_colsum_workspace(int64_t M, int N) { return (int64_t)colsum_row_blocks(M) * N * 4; }

int ecgvit_colsum(const void *in, int64_t ld, float *out, void *partial, int64_t M, int N, int dtype, void *stream) {
    if (M <= 0 || N <= 0 || N % 8 != 0 || ld % 8 != 0 || !partial) return ECGVIT_EINVAL;
    const int rb = colsum_row_blocks(M);
    const int rpb = (int)((M + rb - 1) / rb);
    const int rc = dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        constexpr int WV = 64 * Vec16<T>::N;
        hipLaunchKernelGGL(colsum_kernel<T>, dim3((N + WV - 1) / WV, rb), dim3(256), 0, as_stream(stream), (const T *)in, ld, (float *)partial, M, N, rpb);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
    if (rc != ECGVIT_OK) return rc;
    hipLaunchKernelGGL(reduce_partials_kernel, dim3((N + 63) / 64), dim3(1024), 0, as_stream(stream), (const float *)partial, rb, N, out, out, N);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

static int dropout_apply_launch(const void *in, void *out, int64_t count, float dropout_p, uint64_t seed, int dtype, void *stream, int64_t cols,
                                int64_t mrp) {
    if (count <= 0 || count % 8 != 0 || cols < 8 || cols % 8 != 0 || count % cols != 0 || mrp < 1 || (mrp > 1 && count * mrp >= (1ll << 32)))
        return ECGVIT_EINVAL;
    const int grid = (int)std::min<int64_t>((count / 4 + 255) / 256, 4096);
    return dispatch_dtype(dtype, [&](auto e) -> int {
        using T = decltype(e);
        uint32_t th;
        float ik;
        if (!dropout_site_params(dropout_p, sizeof(T) == 2, th, ik)) return ECGVIT_EINVAL;   // (bf16: p applied as round(256 p) / 256; below 1/512: rejected)
        hipLaunchKernelGGL(dropout_apply_kernel<T>, dim3(grid), dim3(256), 0, as_stream(stream), (const T *)in, (T *)out, count, seed, th, ik, (uint32_t)cols, (uint32_t)mrp);
        ECGVIT_CHECK_LAUNCH();
        return ECGVIT_OK;
    });
}

int ecgvit_dropout_apply(const void *in, void *out, int64_t count, float dropout_p, uint64_t seed, int dtype, void *stream) {
    return dropout_apply_launch(in, out, count, dropout_p, seed, dtype, stream, 8, 1);
}

int ecgvit_dropout_apply_rows(const void *in, void *out, int64_t rows, int cols, int mask_row_pitch, float dropout_p, uint64_t seed, int dtype,
                              void *stream) {
    if (rows <= 0) return ECGVIT_EINVAL;
    return dropout_apply_launch(in, out, rows * cols, dropout_p, seed, dtype, stream, cols, mask_row_pitch);
}

int ecgvit_softmax_rows(float *S, int64_t rows, int N, int64_t ld, void *stream) {
    if (rows <= 0 || N <= 0 || ld < N) return ECGVIT_EINVAL;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3(grid_for_rows(rows)), dim3(256), 0, as_stream(stream), S, rows, N, ld);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_softmax_bwd_rows(const float *P, float *dP, int64_t rows, int N, int64_t ld, float scale, void *stream) {
    if (rows <= 0 || N <= 0 || ld < N) return ECGVIT_EINVAL;
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3(grid_for_rows(rows)), dim3(256), 0, as_stream(stream), P, dP, rows, N, ld, scale);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

}  // extern "C"
