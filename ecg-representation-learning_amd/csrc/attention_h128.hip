// Fused multi-head self-attention for 128-wide heads (bf16, dh = 128, 1 <= N <= 2048): the dh = 128 branches of ecgvit_attention_fwd / _bwd /
// _cls_fwd / _cls_bwd (attention.hip checks the arguments and calls the launchers at the bottom of this file).
//
// Every [row][128 x bf16] operand sits in LDS as TWO standard [row][64] images (dims 0-63 | 64-127), so the swizzle and the fragment readers of
// attn_common.h apply unchanged: a 32 x 32 product over the head dim is 4 MFMAs on each half image, and a 128-row result is 4 accumulators
// (dt = 0, 1 from the low image, 2, 3 from the high one).
//
// Contract shared with the dh = 64 kernels: same qkv / out / lse / dqkv layouts, LSE = m scale + log(sum p) in natural-log units, and the same
// dropout bits -- element (bh, q, key): quad = (bh N + q) ceil(N / 4) + key / 4, byte key & 3, keep iff byte >= round(256 p), kept values
// scaled by 256 / (256 - round(256 p)).  No atomics: every output element is written by exactly one lane, so launches are bit-reproducible.
//
// forward   one 4-wave workgroup per (record, head, 128-query block); each wave owns 32 queries (query on the lane), online softmax over 64-key
//           windows of K and V staged in LDS (S^T = K Q^T, O^T += V^T P^T, lazy running maximum as in attention.hip).
// backward  two kernels, deterministic without atomics:
//           dK / dV  one workgroup per (record, head, 128-key block), key on the lane, loop over 32-query blocks of Q / dO staged in LDS;
//                    dK^T / dV^T of the wave's 32 keys (8 accumulators) live in registers for the whole loop.
//           dQ       one workgroup per (record, head, 128-query block), query on the lane, loop over 64-key windows of K / V in LDS;
//                    P is recomputed from the stored LSE (dS^T = P^T (m dP^T - delta), dQ^T += K^T dS^T).
// CLS row   VALU kernels for query row 0 only (the pruned last block of the supervised step): 256 threads = 16 key slots x 16 lanes of 8 dims.
#include "attn_common.h"
#include "attn_h128.h"

namespace {

constexpr int H128_WK = 64;                 // keys per K / V window (forward, dQ)
constexpr float H128_LOG2E = 1.44269504088896340736f;

// ---- the vector phase of one 32-key x 32-query score tile with four output accumulators (the dh = 64 kernels' attn_fwd_tile_vec with o[4]):
// lazy running maximum (the reference moves only when a tile exceeds it by more than 2^8), p = exp2(s c - m c), row sum, dropout, bf16 pairs
template <bool DROP>
__device__ __forceinline__ void h128_tile_vec(f32x16 &sc, float &m, float &l, f32x16 (&o)[4], float c, uint32_t smix, uint32_t quad0, uint32_t thresh,
                                              u32x4 (&pk)[2]) {
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
        for (int dt = 0; dt < 4; ++dt)
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
        // keys 8 g + 4 lh + k of the tile: quad quad0 + 2 g (quad0 carries the tile and the lane half)
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
__device__ __forceinline__ void h128_store4(bf16_t *dst, const f32x16 &acc, int g, float f) {
    bf16x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (bf16_t)(acc[4 * g + k] * f);
    *reinterpret_cast<bf16x4 *>(dst) = v;
}

// =====================================================================================================
// forward.  Budget: <= 168 VGPRs, three waves per SIMD (Q fragments 32, O^T 4 x 16, scores 16, the staging loads of a window; at 128 it spills),
// no scratch; LDS 32 KiB static (K and V windows of 64 keys, two half images each).  tests/test_head_dim_128.py holds these budgets.
// =====================================================================================================
template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void attn128_fwd_kernel(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out, float *__restrict__ lse,
                                                          int N, int h, float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    constexpr int HB = H128_WK * 128;   // bytes of one half image
    __shared__ __attribute__((aligned(16))) char smem[4 * HB];
    char *const Klo = smem, *const Khi = smem + HB, *const Vlo = smem + 2 * HB, *const Vhi = smem + 3 * HB;
    const int nqb = (N + 127) >> 7;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / h, hd = bh - b * h;
    const int d = h * 128;
    const int64_t d3 = 3 * (int64_t)d;
    const bf16_t *base = qkv + (int64_t)b * N * d3 + hd * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int q = qb * 128 + wave * 32 + lr, qc = q < N ? q : N - 1;
    bf16x8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const bf16x8 *>(base + (int64_t)qc * d3 + ks * 16 + 8 * lh);
    const uint32_t rowquad = ((uint32_t)bh * (uint32_t)N + (uint32_t)qc) * (uint32_t)((N + 3) >> 2);
    const uint32_t smix = seed_mix(seed);
    const float c = scale * H128_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    const int nkt = (N + 31) >> 5;

    f32x16 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < N; k0 += H128_WK) {
        const int nv = min(H128_WK, N - k0), rp = ((nv + 31) >> 5) << 5;
        __syncthreads();   // everyone is done with the previous window
        const bf16_t *kb = base + d + (int64_t)k0 * d3, *vb = base + 2 * d + (int64_t)k0 * d3;
        stage_image<256>(Klo, kb, d3, nv, rp);
        stage_image<256>(Khi, kb + 64, d3, nv, rp);
        stage_image<256>(Vlo, vb, d3, nv, rp);
        stage_image<256>(Vhi, vb + 64, d3, nv, rp);
        __syncthreads();
        for (int ktl = 0; ktl < (rp >> 5); ++ktl) {
            const int kt = (k0 >> 5) + ktl;
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Klo + ktl * 4096, ro.ks[ks]), qf[ks], s, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Khi + ktl * 4096, ro.ks[ks]), qf[4 + ks], s, 0, 0, 0);
            if (kt == nkt - 1) {   // only the last tile holds padded keys
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= N) s[r] = -INFINITY;
                }
            }
            u32x4 pk[2];
            h128_tile_vec<DROP>(s, m, l, o, c, smix, rowquad + (uint32_t)(kt * 8 + lh), thresh, pk);
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pk[ss]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c((dt < 2 ? Vlo : Vhi) + ktl * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]),
                                                                    pf, o[dt], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (q < N) {
        const float inv = inv_keep / l;   // inv_keep = 1 without dropout
        bf16_t *orow = out + ((int64_t)b * N + q) * d + hd * 128;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) h128_store4(orow + dt * 32 + 8 * g + 4 * lh, o[dt], g, inv);
        if (lh == 0) lse[(int64_t)bh * N + q] = m * scale + logf(l);
    }
}

// =====================================================================================================
// backward, dK / dV.  Budget: <= 256 VGPRs, two waves per SIMD (dK^T / dV^T 8 x 16, V fragments 32, S / dP 32; the K fragments are read from an
// LDS image per block: held in registers they spilled), no scratch; LDS 48.25 KiB static (the block's 128 K rows, Q and dO images of one 32-query
// block, LSE and delta of its rows).
// =====================================================================================================
template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn128_bwd_dkv_kernel(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ out,
                                                              const bf16_t *__restrict__ dout, const float *__restrict__ lse,
                                                              bf16_t *__restrict__ dqkv, int N, int h, float scale,
                                                              uint64_t seed, uint32_t thresh, float inv_keep) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 4096 + 2 * 32 * 4 + 2 * 128 * 128];
    char *const Qlo = smem, *const Qhi = smem + 4096, *const Dlo = smem + 8192, *const Dhi = smem + 12288;
    float *const lse_s = reinterpret_cast<float *>(smem + 16384), *const delta_s = lse_s + 32;
    char *const Klo = smem + 16384 + 256, *const Khi = Klo + 128 * 128;   // the block's 128 K rows, read again for every query block
    const int nkb = (N + 127) >> 7;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / h, hd = bh - b * h;
    const int d = h * 128;
    const int64_t d3 = 3 * (int64_t)d;
    const bf16_t *base = qkv + (int64_t)b * N * d3 + hd * 128;
    const bf16_t *obase = out + (int64_t)b * N * d + hd * 128, *dobase = dout + (int64_t)b * N * d + hd * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int mykey = kb * 128 + wave * 32 + lr, kc = mykey < N ? mykey : N - 1;   // (keys >= N: clamped loads, never stored)
    bf16x8 vf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) vf[ks] = *reinterpret_cast<const bf16x8 *>(base + 2 * d + (int64_t)kc * d3 + ks * 16 + 8 * lh);
    {
        const int k0 = kb * 128, nk = min(128, N - k0);
        stage_image<256>(Klo, base + d + (int64_t)k0 * d3, d3, nk, 128);
        stage_image<256>(Khi, base + d + 64 + (int64_t)k0 * d3, d3, nk, 128);
    }   // (visible behind the first block's barriers)
    f32x16 dKt[4], dVt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dKt[dt][r] = 0.f; dVt[dt][r] = 0.f; }
    const float c = scale * H128_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    // dropout: the 4 keys of a quad sit on 4 adjacent lanes (the key block starts at a multiple of 4): lane j of the quad hashes query j of each
    // group of four, the others take the word by a quad_perm broadcast (attention.hip, attn_bwd_bf16_kernel)
    const uint32_t qpitch = (uint32_t)((N + 3) >> 2), hstep = qpitch * ECGVIT_WEYL, smix = seed_mix(seed);
    const uint32_t bsh = (uint32_t)(mykey & 3) * 8u, lq = (uint32_t)(lane & 3);

    for (int q0 = 0; q0 < N; q0 += 32) {
        const int nv = min(32, N - q0);
        __syncthreads();   // everyone is done with the previous block
        stage_image<256>(Qlo, base + (int64_t)q0 * d3, d3, nv, 32);
        stage_image<256>(Qhi, base + 64 + (int64_t)q0 * d3, d3, nv, 32);
        stage_image<256>(Dlo, dobase + (int64_t)q0 * d, d, nv, 32);
        stage_image<256>(Dhi, dobase + 64 + (int64_t)q0 * d, d, nv, 32);
        {   // delta = rowsum(dO * O) and LSE (log2 units) of the block's rows: 8 lanes per row, 16 dims each; rows >= N: 0 (their Q / dO rows are 0)
            const int row = threadIdx.x >> 3, part = threadIdx.x & 7;
            const int r = q0 + row, rc = r < N ? r : N - 1;
            const Vec16<bf16_t> a0 = ld16(dobase + (int64_t)rc * d + part * 16), a1 = ld16(dobase + (int64_t)rc * d + part * 16 + 8);
            const Vec16<bf16_t> o0 = ld16(obase + (int64_t)rc * d + part * 16), o1 = ld16(obase + (int64_t)rc * d + part * 16 + 8);
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) acc += a0.get(k) * o0.get(k) + a1.get(k) * o1.get(k);
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (part == 0) {
                delta_s[row] = r < N ? acc : 0.f;
                lse_s[row] = r < N ? lse[(int64_t)bh * N + rc] * H128_LOG2E : 0.f;
            }
        }
        __syncthreads();
        // S = Q K^T, dP = dO V^T with the key on the lane; rows = queries q0 + 8 (r >> 2) + 4 lh + (r & 3)
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Qlo, ro.ks[ks]), row_frag_c(Klo + wave * 4096, ro.ks[ks]), s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Dlo, ro.ks[ks]), vf[ks], dp, 0, 0, 0);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Qhi, ro.ks[ks]), row_frag_c(Khi + wave * 4096, ro.ks[ks]), s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Dhi, ro.ks[ks]), vf[4 + ks], dp, 0, 0, 0);
        }
        const uint32_t hq0 = smix + (((uint32_t)bh * (uint32_t)N + (uint32_t)q0) * qpitch + (uint32_t)(mykey >> 2)) * ECGVIT_WEYL;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 l4 = *reinterpret_cast<const f32x4 *>(&lse_s[8 * g4 + 4 * lh]);
            const f32x4 d4 = *reinterpret_cast<const f32x4 *>(&delta_s[8 * g4 + 4 * lh]);
            [[maybe_unused]] uint32_t hk[4];
            if constexpr (DROP) {
                const uint32_t mine = pair_finish(hq0 + ((uint32_t)(8 * g4 + 4 * lh) + lq) * hstep);   // query k = lane & 3 of this group
                hk[0] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x00, 0xF, 0xF, true);   // quad_perm:[0,0,0,0]
                hk[1] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x55, 0xF, 0xF, true);   // [1,1,1,1]
                hk[2] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xAA, 0xF, 0xF, true);   // [2,2,2,2]
                hk[3] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0xFF, 0xF, 0xF, true);   // [3,3,3,3]
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = 4 * g4 + k;
                const float p = __builtin_amdgcn_exp2f(s[r] * c - l4[k]);
                float g = dp[r];
                if constexpr (DROP) {
                    const float mlt = ((hk[k] >> bsh) & 0xFFu) >= thresh ? inv_keep : 0.f;
                    g *= mlt;
                    s[r] = p * mlt;   // dropped probabilities feed dV
                } else {
                    s[r] = p;
                }
                dp[r] = p * (g - d4[k]) * scale;   // dS, in place
            }
        }
        // dV^T += dO^T P, dK^T += Q^T dS: A = transposed reads of the dO / Q images, B = the packed P / dS accumulators
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 pf = pack8(s, ss), dsf = pack8(dp, ss);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dVt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c((dt < 2 ? Dlo : Dhi) + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]), pf, dVt[dt], 0, 0, 0);
                dKt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c((dt < 2 ? Qlo : Qhi) + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]), dsf, dKt[dt], 0, 0, 0);
            }
        }
    }
    if (mykey < N) {   // lane = key, accumulator rows = dims dt * 32 + 8 g + 4 lh + 0..3
        bf16_t *dk = dqkv + ((int64_t)b * N + mykey) * d3 + d + hd * 128;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                h128_store4(dk + dt * 32 + 8 * g + 4 * lh, dKt[dt], g, 1.f);
                h128_store4(dk + d + dt * 32 + 8 * g + 4 * lh, dVt[dt], g, 1.f);
            }
    }
}

// =====================================================================================================
// backward, dQ (P recomputed).  Budget: <= 256 VGPRs, two waves per SIMD (Q and dO fragments 64, dQ^T 4 x 16, S^T / dP^T 32), no scratch; LDS
// 32 KiB static (K and V windows of 64 keys, as the forward).
// =====================================================================================================
template <bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void attn128_bwd_dq_kernel(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ out,
                                                             const bf16_t *__restrict__ dout, const float *__restrict__ lse,
                                                             bf16_t *__restrict__ dqkv, int N, int h, float scale,
                                                             uint64_t seed, uint32_t thresh, float inv_keep) {
    constexpr int HB = H128_WK * 128;
    __shared__ __attribute__((aligned(16))) char smem[4 * HB];
    char *const Klo = smem, *const Khi = smem + HB, *const Vlo = smem + 2 * HB, *const Vhi = smem + 3 * HB;
    const int nqb = (N + 127) >> 7;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / h, hd = bh - b * h;
    const int d = h * 128;
    const int64_t d3 = 3 * (int64_t)d;
    const bf16_t *base = qkv + (int64_t)b * N * d3 + hd * 128;
    const bf16_t *obase = out + (int64_t)b * N * d + hd * 128, *dobase = dout + (int64_t)b * N * d + hd * 128;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int q = qb * 128 + wave * 32 + lr, qc = q < N ? q : N - 1;
    bf16x8 qf[8], dof[8];
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        qf[ks] = *reinterpret_cast<const bf16x8 *>(base + (int64_t)qc * d3 + ks * 16 + 8 * lh);
        dof[ks] = *reinterpret_cast<const bf16x8 *>(dobase + (int64_t)qc * d + ks * 16 + 8 * lh);
        const bf16x8 of = *reinterpret_cast<const bf16x8 *>(obase + (int64_t)qc * d + ks * 16 + 8 * lh);
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += (float)dof[ks][j] * (float)of[j];
    }
    delta += __shfl_xor(delta, 32, 64);   // the two lane halves hold the two halves of every 16-dim step
    const float lse2 = lse[(int64_t)bh * N + qc] * H128_LOG2E;
    const uint32_t rowquad = ((uint32_t)bh * (uint32_t)N + (uint32_t)qc) * (uint32_t)((N + 3) >> 2);
    const uint32_t smix = seed_mix(seed);
    const float c = scale * H128_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    const int nkt = (N + 31) >> 5;

    f32x16 dQt[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQt[dt][r] = 0.f;
    for (int k0 = 0; k0 < N; k0 += H128_WK) {
        const int nv = min(H128_WK, N - k0), rp = ((nv + 31) >> 5) << 5;
        __syncthreads();
        const bf16_t *kb = base + d + (int64_t)k0 * d3, *vb = base + 2 * d + (int64_t)k0 * d3;
        stage_image<256>(Klo, kb, d3, nv, rp);
        stage_image<256>(Khi, kb + 64, d3, nv, rp);
        stage_image<256>(Vlo, vb, d3, nv, rp);
        stage_image<256>(Vhi, vb + 64, d3, nv, rp);
        __syncthreads();
        for (int ktl = 0; ktl < (rp >> 5); ++ktl) {
            const int kt = (k0 >> 5) + ktl;
            // S^T = K Q^T, dP^T = V dO^T: key on the accumulator row (8 (r >> 2) + 4 lh + (r & 3)), query on the lane
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Klo + ktl * 4096, ro.ks[ks]), qf[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Vlo + ktl * 4096, ro.ks[ks]), dof[ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Khi + ktl * 4096, ro.ks[ks]), qf[4 + ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Vhi + ktl * 4096, ro.ks[ks]), dof[4 + ks], dp, 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                [[maybe_unused]] uint32_t hh = 0u;
                if constexpr (DROP) hh = quad_hash(smix, rowquad + (uint32_t)(kt * 8 + 2 * g + lh));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 4 * g + k;
                    float p = __builtin_amdgcn_exp2f(s[r] * c - lse2);
                    if (kt == nkt - 1 && kt * 32 + 8 * g + 4 * lh + k >= N) p = 0.f;
                    float gp = dp[r];
                    if constexpr (DROP) gp *= ((hh >> (8 * k)) & 0xFFu) >= thresh ? inv_keep : 0.f;
                    s[r] = p * (gp - delta);   // dS^T / scale
                }
            }
            // dQ^T += K^T dS^T: A = transposed reads of the K image, B = the packed dS^T accumulator (the forward's O^T += V^T P^T)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 dsf = pack8(s, ss);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    dQt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c((dt < 2 ? Klo : Khi) + ktl * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]),
                                                                      dsf, dQt[dt], 0, 0, 0);
            }
        }
    }
    if (q < N) {
        bf16_t *dq = dqkv + ((int64_t)b * N + q) * d3 + hd * 128;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) h128_store4(dq + dt * 32 + 8 * g + 4 * lh, dQt[dt], g, scale);
    }
}

// =====================================================================================================
// CLS row (query 0 of each record), dh = 128: one workgroup per (record, head), 16 key slots x 16 lanes, each lane 8 of the 128 dims.  The same
// arithmetic as attention.hip's attn_cls_fwd_kernel / attn_cls_bwd_kernel; bandwidth kernels, no MFMA.  LDS 16.3 KiB (fwd) / 8.3 KiB (bwd).
// =====================================================================================================
constexpr int C128_THREADS = 256, C128_SLOTS = 16, C128_NMAX = ECGVIT_ATTN_MAX_N;
__device__ __forceinline__ float group16_sum(float v) {   // sum over the 16 lanes that share a key slot
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}
template <bool DROP> __device__ __forceinline__ float c128_mult(uint32_t smix, uint32_t quad0, int key, uint32_t thresh, float inv_keep) {
    if constexpr (!DROP) return 1.f;
    const uint32_t hsh = quad_hash(smix, quad0 + (uint32_t)(key >> 2));
    return ((hsh >> (8 * (key & 3))) & 0xFFu) >= thresh ? inv_keep : 0.f;
}
template <bool MAX> __device__ __forceinline__ float c128_block_reduce(float v, float *red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = MAX ? fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) : (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return r;
}

template <bool DROP>
__global__ __launch_bounds__(C128_THREADS) void attn128_cls_fwd_kernel(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out, float *__restrict__ lse,
                                                                       int N, int h, float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    __shared__ float sp[C128_NMAX];              // scores, then dropped probabilities, per key
    __shared__ float ored[C128_SLOTS][129];      // per-slot partial outputs
    __shared__ float red[4];
    const int bh = blockIdx.x, b = bh / h, head = bh % h;
    const int g = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int64_t dm = (int64_t)h * 128, ld = 3 * dm;
    const bf16_t *rec = qkv + (int64_t)b * N * ld + head * 128 + g * 8;
    const Vec16<bf16_t> q = ld16(rec);
    float smax = -INFINITY;
    for (int k = slot; k < N; k += C128_SLOTS) {
        const Vec16<bf16_t> kv = ld16(rec + (int64_t)k * ld + dm);
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = fmaf(q.get(t), kv.get(t), acc);
        acc = group16_sum(acc) * scale;
        if (g == 0) sp[k] = acc;
        smax = fmaxf(smax, acc);
    }
    const float m = c128_block_reduce<true>(smax, red);
    float ssum = 0.f;
    for (int k = threadIdx.x; k < N; k += C128_THREADS) ssum += __expf(sp[k] - m);
    const float l = m + __logf(c128_block_reduce<false>(ssum, red));
    const uint32_t smix = seed_mix(seed), quad0 = (uint32_t)bh * (uint32_t)N * (uint32_t)((N + 3) >> 2);
    for (int k = threadIdx.x; k < N; k += C128_THREADS) sp[k] = __expf(sp[k] - l) * c128_mult<DROP>(smix, quad0, k, thresh, inv_keep);
    __syncthreads();
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = slot; k < N; k += C128_SLOTS) {
        const Vec16<bf16_t> vv = ld16(rec + (int64_t)k * ld + 2 * dm);
        const float p = sp[k];
#pragma unroll
        for (int t = 0; t < 8; ++t) o[t] = fmaf(p, vv.get(t), o[t]);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) ored[slot][g * 8 + t] = o[t];
    __syncthreads();
    if (threadIdx.x < 128) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < C128_SLOTS; ++j) s += ored[j][threadIdx.x];
        out[(int64_t)b * dm + head * 128 + threadIdx.x] = (bf16_t)s;
        if (threadIdx.x == 0) lse[bh] = l;
    }
}

template <bool DROP>
__global__ __launch_bounds__(C128_THREADS) void attn128_cls_bwd_kernel(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ o_cls,
                                                                       const bf16_t *__restrict__ do_cls, const float *__restrict__ lse,
                                                                       bf16_t *__restrict__ dqkv, bf16_t *__restrict__ dq_cls, int N, int h, float scale,
                                                                       uint64_t seed, uint32_t thresh, float inv_keep) {
    __shared__ float qred[C128_SLOTS][129];
    const int bh = blockIdx.x, b = bh / h, head = bh % h;
    const int g = threadIdx.x & 15, slot = threadIdx.x >> 4;
    const int64_t dm = (int64_t)h * 128, ld = 3 * dm;
    const int64_t roff = (int64_t)b * N * ld + head * 128 + g * 8;
    const bf16_t *rec = qkv + roff;
    bf16_t *drec = dqkv + roff;
    const Vec16<bf16_t> q = ld16(rec), dO = ld16(do_cls + (int64_t)b * dm + head * 128 + g * 8), O = ld16(o_cls + (int64_t)b * dm + head * 128 + g * 8);
    float D = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) D = fmaf(dO.get(t), O.get(t), D);
    D = group16_sum(D);
    const float l = lse[bh];
    const uint32_t smix = seed_mix(seed), quad0 = (uint32_t)bh * (uint32_t)N * (uint32_t)((N + 3) >> 2);
    float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = slot; k < N; k += C128_SLOTS) {
        const Vec16<bf16_t> kv = ld16(rec + (int64_t)k * ld + dm), vv = ld16(rec + (int64_t)k * ld + 2 * dm);
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) { s = fmaf(q.get(t), kv.get(t), s); dp = fmaf(dO.get(t), vv.get(t), dp); }
        s = group16_sum(s);
        dp = group16_sum(dp);
        const float p = __expf(s * scale - l), mlt = c128_mult<DROP>(smix, quad0, k, thresh, inv_keep);
        const float ds = p * (dp * mlt - D), pm = p * mlt;
        Vec16<bf16_t> dk, dv;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            dq[t] = fmaf(ds, kv.get(t), dq[t]);
            dk.set(t, scale * ds * q.get(t));
            dv.set(t, pm * dO.get(t));
        }
        st16(drec + (int64_t)k * ld + dm, dk);
        st16(drec + (int64_t)k * ld + 2 * dm, dv);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) qred[slot][g * 8 + t] = dq[t];
    __syncthreads();
    if (threadIdx.x < 128) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < C128_SLOTS; ++j) s += qred[j][threadIdx.x];
        dq_cls[(int64_t)b * dm + head * 128 + threadIdx.x] = (bf16_t)(s * scale);
    }
}

}  // namespace

// ---- launchers (arguments already checked by attention.hip: bf16, 1 <= N <= 2048, B, h >= 1, 16-B aligned pointers, dropout threshold)
static bool h128_grid_ok(int B, int h, int per_bh) { return (int64_t)B * h * per_bh < (1ll << 31); }

int attn_h128_fwd(const void *qkv, void *out, float *lse, int B, int N, int h, float scale, uint64_t seed, uint32_t th, float ik, void *stream) {
    const int nqb = (N + 127) / 128;
    if (!h128_grid_ok(B, h, nqb)) return ECGVIT_EINVAL;
    const dim3 grid((unsigned)(B * h * nqb));
#define FWD(DR) hipLaunchKernelGGL(attn128_fwd_kernel<DR>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, (bf16_t *)out, lse, N, h, scale, seed, th, ik)
    if (th) FWD(true); else FWD(false);
#undef FWD
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int attn_h128_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, int B, int N, int h, float scale, uint64_t seed,
                  uint32_t th, float ik, void *stream) {
    const int nb = (N + 127) / 128;   // 128-key blocks (dK / dV) = 128-query blocks (dQ)
    if (!h128_grid_ok(B, h, nb)) return ECGVIT_EINVAL;
    const dim3 grid((unsigned)(B * h * nb));
#define BWD(K, DR) hipLaunchKernelGGL(K<DR>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)qkv, (const bf16_t *)out, (const bf16_t *)dout, lse, \
                                      (bf16_t *)dqkv, N, h, scale, seed, th, ik)
    if (th) BWD(attn128_bwd_dkv_kernel, true); else BWD(attn128_bwd_dkv_kernel, false);
    ECGVIT_CHECK_LAUNCH();
    if (th) BWD(attn128_bwd_dq_kernel, true); else BWD(attn128_bwd_dq_kernel, false);
    ECGVIT_CHECK_LAUNCH();
#undef BWD
    return ECGVIT_OK;
}

int attn_h128_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, int B, int N, int h, float scale, uint64_t seed, uint32_t th, float ik, void *stream) {
#define CLS_FWD(DR) hipLaunchKernelGGL(attn128_cls_fwd_kernel<DR>, dim3(B * h), dim3(C128_THREADS), 0, as_stream(stream), (const bf16_t *)qkv, (bf16_t *)out_cls, \
                                       lse_cls, N, h, scale, seed, th, ik)
    if (th) CLS_FWD(true); else CLS_FWD(false);
#undef CLS_FWD
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int attn_h128_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls, int B, int N, int h,
                      float scale, uint64_t seed, uint32_t th, float ik, void *stream) {
#define CLS_BWD(DR) hipLaunchKernelGGL(attn128_cls_bwd_kernel<DR>, dim3(B * h), dim3(C128_THREADS), 0, as_stream(stream), (const bf16_t *)qkv, \
                                       (const bf16_t *)out_cls, (const bf16_t *)dout_cls, lse_cls, (bf16_t *)dqkv, (bf16_t *)dq_cls, N, h, scale, seed, th, ik)
    if (th) CLS_BWD(true); else CLS_BWD(false);
#undef CLS_BWD
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
