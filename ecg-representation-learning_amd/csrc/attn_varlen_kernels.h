// The fused attention kernels of attention_varlen.hip, written once and included three times (no include guard):
//   AV_FORM 0 -> attnu_*: uniform batch, record b owns rows [b N, b N + N) of qkv / out / dqkv and n = N (no n_tok / tok_off argument: the
//                padding branches fold away at compile time);
//   AV_FORM 1 -> attnv_*: padded batch, the same rows, rows >= n_tok[b] are padding, written as zeros;
//   AV_FORM 2 -> attnr_*: ragged batch, record b owns rows [tok_off[b], tok_off[b] + n_tok[b]) -- packed, no padded rows: nothing past
//                n_tok[b] is read or written.  N is then the widest record's token count (grid, LSE layout, dropout hashing).
// Each form is its own __global__ body, so each compiles exactly as it would alone (a shared __device__ body inlined into several kernels does
// not: the inlined code is scheduled and allocated differently).
#if AV_FORM == 0
#define AV_KERNEL(name) attnu_##name
#define AV_LENGTHS
#define AV_ROW_BASE constexpr bool UN = true, PK = false; const int32_t *const n_tok = nullptr, *const tok_off = nullptr;
#elif AV_FORM == 1
#define AV_KERNEL(name) attnv_##name
#define AV_LENGTHS const int32_t *__restrict__ n_tok,
#define AV_ROW_BASE constexpr bool UN = false, PK = false; const int32_t *const tok_off = nullptr;
#else
#define AV_KERNEL(name) attnr_##name
#define AV_LENGTHS const int32_t *__restrict__ n_tok, const int32_t *__restrict__ tok_off,
#define AV_ROW_BASE constexpr bool UN = false, PK = true;
#endif

// =====================================================================================================
// forward.  Budget: HI = 2: <= 168 VGPRs (three waves per SIMD), HI = 1: <= 128 (four); no scratch; LDS 16 KiB x HI static (K and V windows
// of 64 keys, HI images each).  tests/test_varlen.py holds these budgets.
// =====================================================================================================
template <int HI, bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HI == 1 ? 4 : 3))) void AV_KERNEL(fwd_kernel)(
    const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out, float *__restrict__ lse, AV_LENGTHS int N, int h,
    float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    AV_ROW_BASE
    constexpr int HB = AV_WK * 128, DH = 64 * HI;
    __shared__ __attribute__((aligned(16))) char smem[2 * HI * HB];
    char *const Kimg = smem, *const Vimg = smem + HI * HB;   // image i of K at Kimg + i HB
    const int nqb = (N + 127) >> 7;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / h, hd = bh - b * h;
    const int n = UN ? N : n_tok[b];
    const int d = h * DH;
    const int64_t d3 = 3 * (int64_t)d;
    if (!UN && qb * 128 >= n) {   // every query of the block is padding (packed: does not exist)
        if constexpr (!PK) {
            const int r1 = min(qb * 128 + 128, N);
            av_zero_rows<DH>(out + (int64_t)b * N * d + hd * DH, d, qb * 128, r1);
            for (int r = qb * 128 + (int)threadIdx.x; r < r1; r += 256) lse[(int64_t)bh * N + r] = 0.f;
        }
        return;
    }
    const bf16_t *base = PK ? qkv + (int64_t)tok_off[b] * d3 + hd * DH : qkv + (int64_t)b * N * d3 + hd * DH;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int q = qb * 128 + wave * 32 + lr, qc = q < n ? q : n - 1;
    bf16x8 qf[4 * HI];
#pragma unroll
    for (int ks = 0; ks < 4 * HI; ++ks) qf[ks] = *reinterpret_cast<const bf16x8 *>(base + (int64_t)qc * d3 + ks * 16 + 8 * lh);
    const uint32_t rowquad = ((uint32_t)bh * (uint32_t)N + (uint32_t)qc) * (uint32_t)((N + 3) >> 2);
    const uint32_t smix = seed_mix(seed);
    const float c = scale * AV_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    const int nkt = (n + 31) >> 5;

    f32x16 o[2 * HI];
#pragma unroll
    for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < n; k0 += AV_WK) {
        const int nv = min(AV_WK, n - k0), rp = ((nv + 31) >> 5) << 5;
        __syncthreads();   // everyone is done with the previous window
        const bf16_t *kb = base + d + (int64_t)k0 * d3, *vb = base + 2 * d + (int64_t)k0 * d3;
#pragma unroll
        for (int i = 0; i < HI; ++i) {
            stage_image<256>(Kimg + i * HB, kb + 64 * i, d3, nv, rp);
            stage_image<256>(Vimg + i * HB, vb + 64 * i, d3, nv, rp);
        }
        __syncthreads();
        for (int ktl = 0; ktl < (rp >> 5); ++ktl) {
            const int kt = (k0 >> 5) + ktl;
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int i = 0; i < HI; ++i)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Kimg + i * HB + ktl * 4096, ro.ks[ks]), qf[4 * i + ks], s, 0, 0, 0);
            if (kt == nkt - 1) {   // only the last tile holds keys past n
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    if (key >= n) s[r] = -INFINITY;
                }
            }
            u32x4 pk[2];
            av_tile_vec<HI, DROP>(s, m, l, o, c, smix, rowquad + (uint32_t)(kt * 8 + lh), thresh, pk);
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pk[ss]);
#pragma unroll
                for (int dt = 0; dt < 2 * HI; ++dt)
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        tr_frag_c(Vimg + (dt >> 1) * HB + ktl * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]), pf, o[dt], 0, 0, 0);
            }
        }
    }
    l += __shfl_xor(l, 32, 64);
    if (q < (PK ? n : N)) {
        const bool valid = UN || q < n;
        const float inv = inv_keep / l;   // inv_keep = 1 without dropout
        bf16_t *orow = PK ? out + ((int64_t)tok_off[b] + q) * d + hd * DH : out + ((int64_t)b * N + q) * d + hd * DH;
#pragma unroll
        for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (valid) av_store4(orow + dt * 32 + 8 * g + 4 * lh, o[dt], g, inv);
                else av_zero4(orow + dt * 32 + 8 * g + 4 * lh);
            }
        if (lh == 0) lse[(int64_t)bh * N + q] = valid ? m * scale + logf(l) : 0.f;
    }
}

// =====================================================================================================
// backward, dK / dV: one workgroup per (record, head, 128-key block), key on the lane, loop over the 32-query blocks of Q / dO below n_tok.
// Budget: <= 256 VGPRs (two waves per SIMD), no scratch; LDS HI x 24 KiB + 256 B static (the block's 128 K rows, Q and dO images of one
// 32-query block, LSE and delta of its rows).
// =====================================================================================================
template <int HI, bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void AV_KERNEL(bwd_dkv_kernel)(
    const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ out, const bf16_t *__restrict__ dout, const float *__restrict__ lse,
    bf16_t *__restrict__ dqkv, AV_LENGTHS int N, int h, float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    AV_ROW_BASE
    constexpr int DH = 64 * HI;
    __shared__ __attribute__((aligned(16))) char smem[2 * HI * 4096 + 2 * 32 * 4 + HI * 128 * 128];
    char *const Qimg = smem, *const Dimg = smem + HI * 4096;   // image i at + i 4096
    float *const lse_s = reinterpret_cast<float *>(smem + 2 * HI * 4096), *const delta_s = lse_s + 32;
    char *const Kimg = smem + 2 * HI * 4096 + 256;              // image i at + i 16384
    const int nkb = (N + 127) >> 7;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / h, hd = bh - b * h;
    const int n = UN ? N : n_tok[b];
    const int d = h * DH;
    const int64_t d3 = 3 * (int64_t)d;
    if (!UN && kb * 128 >= n) {   // every key of the block is padding: dK = dV = 0 (packed: does not exist)
        if constexpr (!PK) {
            const int r1 = min(kb * 128 + 128, N);
            bf16_t *dk = dqkv + (int64_t)b * N * d3 + d + hd * DH;
            av_zero_rows<DH>(dk, d3, kb * 128, r1);
            av_zero_rows<DH>(dk + d, d3, kb * 128, r1);
        }
        return;
    }
    const bf16_t *base = PK ? qkv + (int64_t)tok_off[b] * d3 + hd * DH : qkv + (int64_t)b * N * d3 + hd * DH;
    const bf16_t *obase = PK ? out + (int64_t)tok_off[b] * d + hd * DH : out + (int64_t)b * N * d + hd * DH,
                 *dobase = PK ? dout + (int64_t)tok_off[b] * d + hd * DH : dout + (int64_t)b * N * d + hd * DH;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int mykey = kb * 128 + wave * 32 + lr, kc = mykey < n ? mykey : n - 1;   // (keys >= n: clamped loads, zeros stored)
    bf16x8 vf[4 * HI];
#pragma unroll
    for (int ks = 0; ks < 4 * HI; ++ks) vf[ks] = *reinterpret_cast<const bf16x8 *>(base + 2 * d + (int64_t)kc * d3 + ks * 16 + 8 * lh);
    {
        const int k0 = kb * 128, nk = min(128, n - k0);
#pragma unroll
        for (int i = 0; i < HI; ++i) stage_image<256>(Kimg + i * 16384, base + d + 64 * i + (int64_t)k0 * d3, d3, nk, 128);
    }   // (visible behind the first block's barriers)
    f32x16 dKt[2 * HI], dVt[2 * HI];
#pragma unroll
    for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dKt[dt][r] = 0.f; dVt[dt][r] = 0.f; }
    const float c = scale * AV_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    // dropout: the 4 keys of a quad sit on 4 adjacent lanes (the key block starts at a multiple of 4): lane j of the quad hashes query j of each
    // group of four, the others take the word by a quad_perm broadcast
    const uint32_t qpitch = (uint32_t)((N + 3) >> 2), hstep = qpitch * ECGVIT_WEYL, smix = seed_mix(seed);
    const uint32_t bsh = (uint32_t)(mykey & 3) * 8u, lq = (uint32_t)(lane & 3);

    for (int q0 = 0; q0 < n; q0 += 32) {
        const int nv = min(32, n - q0);
        __syncthreads();   // everyone is done with the previous block
#pragma unroll
        for (int i = 0; i < HI; ++i) {
            stage_image<256>(Qimg + i * 4096, base + 64 * i + (int64_t)q0 * d3, d3, nv, 32);
            stage_image<256>(Dimg + i * 4096, dobase + 64 * i + (int64_t)q0 * d, d, nv, 32);
        }
        {   // delta = rowsum(dO * O) and LSE (log2 units) of the block's rows: 8 lanes per row, 8 HI dims each; rows >= n: 0 (their Q / dO rows are 0)
            const int row = threadIdx.x >> 3, part = threadIdx.x & 7;
            const int r = q0 + row, rc = r < n ? r : n - 1;
            Vec16<bf16_t> a[HI], o[HI];
#pragma unroll
            for (int i = 0; i < HI; ++i) {
                a[i] = ld16(dobase + (int64_t)rc * d + part * 8 * HI + 8 * i);
                o[i] = ld16(obase + (int64_t)rc * d + part * 8 * HI + 8 * i);
            }
            float acc = 0.f;   // (one expression per k: the summation order every form shares)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if constexpr (HI == 1) acc += a[0].get(k) * o[0].get(k);
                else acc += a[0].get(k) * o[0].get(k) + a[1].get(k) * o[1].get(k);
            }
            acc += __shfl_xor(acc, 1, 64);
            acc += __shfl_xor(acc, 2, 64);
            acc += __shfl_xor(acc, 4, 64);
            if (part == 0) {
                delta_s[row] = r < n ? acc : 0.f;
                lse_s[row] = r < n ? lse[(int64_t)bh * N + rc] * AV_LOG2E : 0.f;
            }
        }
        __syncthreads();
        // S = Q K^T, dP = dO V^T with the key on the lane; rows = queries q0 + 8 (r >> 2) + 4 lh + (r & 3)
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
        for (int i = 0; i < HI; ++i)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Qimg + i * 4096, ro.ks[ks]), row_frag_c(Kimg + i * 16384 + wave * 4096, ro.ks[ks]), s,
                                                            0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Dimg + i * 4096, ro.ks[ks]), vf[4 * i + ks], dp, 0, 0, 0);
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
            for (int dt = 0; dt < 2 * HI; ++dt) {
                dVt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c(Dimg + (dt >> 1) * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]), pf, dVt[dt], 0, 0, 0);
                dKt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c(Qimg + (dt >> 1) * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]), dsf, dKt[dt], 0, 0, 0);
            }
        }
    }
    if (mykey < (PK ? n : N)) {   // lane = key, accumulator rows = dims dt * 32 + 8 g + 4 lh + 0..3
        const bool valid = UN || mykey < n;
        bf16_t *dk = PK ? dqkv + ((int64_t)tok_off[b] + mykey) * d3 + d + hd * DH : dqkv + ((int64_t)b * N + mykey) * d3 + d + hd * DH;
#pragma unroll
        for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16_t *pk = dk + dt * 32 + 8 * g + 4 * lh, *pv = pk + d;
                if (valid) { av_store4(pk, dKt[dt], g, 1.f); av_store4(pv, dVt[dt], g, 1.f); }
                else { av_zero4(pk); av_zero4(pv); }
            }
    }
}

// =====================================================================================================
// backward, dQ (P recomputed): one workgroup per (record, head, 128-query block), query on the lane, loop over 64-key windows below n_tok.
// Budget: <= 256 VGPRs (two waves per SIMD), no scratch; LDS 16 KiB x HI static (K and V windows of 64 keys, as the forward).
// =====================================================================================================
template <int HI, bool DROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void AV_KERNEL(bwd_dq_kernel)(
    const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ out, const bf16_t *__restrict__ dout, const float *__restrict__ lse,
    bf16_t *__restrict__ dqkv, AV_LENGTHS int N, int h, float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    AV_ROW_BASE
    constexpr int HB = AV_WK * 128, DH = 64 * HI;
    __shared__ __attribute__((aligned(16))) char smem[2 * HI * HB];
    char *const Kimg = smem, *const Vimg = smem + HI * HB;
    const int nqb = (N + 127) >> 7;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / h, hd = bh - b * h;
    const int n = UN ? N : n_tok[b];
    const int d = h * DH;
    const int64_t d3 = 3 * (int64_t)d;
    if (!UN && qb * 128 >= n) {   // every query of the block is padding: dQ = 0 (packed: does not exist)
        if constexpr (!PK) av_zero_rows<DH>(dqkv + (int64_t)b * N * d3 + hd * DH, d3, qb * 128, min(qb * 128 + 128, N));
        return;
    }
    const bf16_t *base = PK ? qkv + (int64_t)tok_off[b] * d3 + hd * DH : qkv + (int64_t)b * N * d3 + hd * DH;
    const bf16_t *obase = PK ? out + (int64_t)tok_off[b] * d + hd * DH : out + (int64_t)b * N * d + hd * DH,
                 *dobase = PK ? dout + (int64_t)tok_off[b] * d + hd * DH : dout + (int64_t)b * N * d + hd * DH;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 31, lh = lane >> 5;
    const int q = qb * 128 + wave * 32 + lr, qc = q < n ? q : n - 1;
    bf16x8 qf[4 * HI], dof[4 * HI];
    float delta = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4 * HI; ++ks) {
        qf[ks] = *reinterpret_cast<const bf16x8 *>(base + (int64_t)qc * d3 + ks * 16 + 8 * lh);
        dof[ks] = *reinterpret_cast<const bf16x8 *>(dobase + (int64_t)qc * d + ks * 16 + 8 * lh);
        const bf16x8 of = *reinterpret_cast<const bf16x8 *>(obase + (int64_t)qc * d + ks * 16 + 8 * lh);
#pragma unroll
        for (int j = 0; j < 8; ++j) delta += (float)dof[ks][j] * (float)of[j];
    }
    delta += __shfl_xor(delta, 32, 64);   // the two lane halves hold the two halves of every 16-dim step
    const float lse2 = lse[(int64_t)bh * N + qc] * AV_LOG2E;
    const uint32_t rowquad = ((uint32_t)bh * (uint32_t)N + (uint32_t)qc) * (uint32_t)((N + 3) >> 2);
    const uint32_t smix = seed_mix(seed);
    const float c = scale * AV_LOG2E;
    const RowOff ro = make_row_off(lane);
    const TrOff to = make_tr_off(lane);
    const int nkt = (n + 31) >> 5;

    f32x16 dQt[2 * HI];
#pragma unroll
    for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dQt[dt][r] = 0.f;
    for (int k0 = 0; k0 < n; k0 += AV_WK) {
        const int nv = min(AV_WK, n - k0), rp = ((nv + 31) >> 5) << 5;
        __syncthreads();
        const bf16_t *kb = base + d + (int64_t)k0 * d3, *vb = base + 2 * d + (int64_t)k0 * d3;
#pragma unroll
        for (int i = 0; i < HI; ++i) {
            stage_image<256>(Kimg + i * HB, kb + 64 * i, d3, nv, rp);
            stage_image<256>(Vimg + i * HB, vb + 64 * i, d3, nv, rp);
        }
        __syncthreads();
        for (int ktl = 0; ktl < (rp >> 5); ++ktl) {
            const int kt = (k0 >> 5) + ktl;
            // S^T = K Q^T, dP^T = V dO^T: key on the accumulator row (8 (r >> 2) + 4 lh + (r & 3)), query on the lane
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int i = 0; i < HI; ++i)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Kimg + i * HB + ktl * 4096, ro.ks[ks]), qf[4 * i + ks], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(row_frag_c(Vimg + i * HB + ktl * 4096, ro.ks[ks]), dof[4 * i + ks], dp, 0, 0, 0);
                }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                [[maybe_unused]] uint32_t hh = 0u;
                if constexpr (DROP) hh = quad_hash(smix, rowquad + (uint32_t)(kt * 8 + 2 * g + lh));
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int r = 4 * g + k;
                    float p = __builtin_amdgcn_exp2f(s[r] * c - lse2);
                    if (kt == nkt - 1 && kt * 32 + 8 * g + 4 * lh + k >= n) p = 0.f;
                    float gp = dp[r];
                    if constexpr (DROP) gp *= ((hh >> (8 * k)) & 0xFFu) >= thresh ? inv_keep : 0.f;
                    s[r] = p * (gp - delta);   // dS^T / scale
                }
            }
            // dQ^T += K^T dS^T: A = transposed reads of the K image, B = the packed dS^T accumulator
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const bf16x8 dsf = pack8(s, ss);
#pragma unroll
                for (int dt = 0; dt < 2 * HI; ++dt)
                    dQt[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_frag_c(Kimg + (dt >> 1) * HB + ktl * 4096 + ss * 2048, to.lo[dt & 1], to.hi[dt & 1]),
                                                                      dsf, dQt[dt], 0, 0, 0);
            }
        }
    }
    if (q < (PK ? n : N)) {
        const bool valid = UN || q < n;
        bf16_t *dq = PK ? dqkv + ((int64_t)tok_off[b] + q) * d3 + hd * DH : dqkv + ((int64_t)b * N + q) * d3 + hd * DH;
#pragma unroll
        for (int dt = 0; dt < 2 * HI; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (valid) av_store4(dq + dt * 32 + 8 * g + 4 * lh, dQt[dt], g, scale);
                else av_zero4(dq + dt * 32 + 8 * g + 4 * lh);
            }
    }
}

// =====================================================================================================
// CLS row (query 0 of each record) against its n keys -- the pruned last block of the supervised step: the classifier reads x[:, 0] only, so
// after the last block's K / V nothing else of that block reaches the loss.  One workgroup per (record, head), 256 threads = 256 / (8 HI) key
// slots x 8 HI lanes of 8 dims (one 16-B load per key row and operand); bandwidth kernels, no MFMA.  The dropout bits are the full kernels'
// for query 0.  The backward writes dK / dV of every key row and a compact dQ.  Budget: <= 128 VGPRs, no scratch; LDS fwd 8 KiB (the
// ECGVIT_ATTN_MAX_N-key score array, at every N) + slots x (DH + 1) floats, bwd slots x (DH + 1) floats.
// =====================================================================================================
template <int HI, bool DROP>
__global__ __launch_bounds__(256) void AV_KERNEL(cls_fwd_kernel)(const bf16_t *__restrict__ qkv, bf16_t *__restrict__ out, float *__restrict__ lse,
                                                        AV_LENGTHS int N, int h, float scale, uint64_t seed,
                                                        uint32_t thresh, float inv_keep) {
    AV_ROW_BASE
    constexpr int DH = 64 * HI, G = 8 * HI, SLOTS = 256 / G;
    __shared__ float sp[AVC_NMAX];          // scores, then dropped probabilities, per key
    __shared__ float ored[SLOTS][DH + 1];   // per-slot partial outputs
    __shared__ float red[4];
    const int bh = blockIdx.x, b = bh / h, head = bh % h;
    const int n = UN ? N : n_tok[b];
    const int g = threadIdx.x % G, slot = threadIdx.x / G;
    const int64_t dm = (int64_t)h * DH, ld = 3 * dm;
    const bf16_t *rec = PK ? qkv + (int64_t)tok_off[b] * ld + head * DH + g * 8 : qkv + (int64_t)b * N * ld + head * DH + g * 8;
    const Vec16<bf16_t> q = ld16(rec);
    float smax = -INFINITY;
    for (int k = slot; k < n; k += SLOTS) {
        const Vec16<bf16_t> kv = ld16(rec + (int64_t)k * ld + dm);
        float acc = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = fmaf(q.get(t), kv.get(t), acc);
        acc = avc_group_sum<HI>(acc) * scale;
        if (g == 0) sp[k] = acc;
        smax = fmaxf(smax, acc);
    }
    const float m = avc_block_reduce<true>(smax, red);
    float ssum = 0.f;
    for (int k = threadIdx.x; k < n; k += 256) ssum += __expf(sp[k] - m);
    const float l = m + __logf(avc_block_reduce<false>(ssum, red));
    const uint32_t smix = seed_mix(seed), quad0 = (uint32_t)bh * (uint32_t)N * (uint32_t)((N + 3) >> 2);
    for (int k = threadIdx.x; k < n; k += 256) sp[k] = __expf(sp[k] - l) * avc_mult<DROP>(smix, quad0, k, thresh, inv_keep);
    __syncthreads();
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = slot; k < n; k += SLOTS) {
        const Vec16<bf16_t> vv = ld16(rec + (int64_t)k * ld + 2 * dm);
        const float p = sp[k];
#pragma unroll
        for (int t = 0; t < 8; ++t) o[t] = fmaf(p, vv.get(t), o[t]);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) ored[slot][g * 8 + t] = o[t];
    __syncthreads();
    if (threadIdx.x < DH) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < SLOTS; ++j) s += ored[j][threadIdx.x];
        out[(int64_t)b * dm + head * DH + threadIdx.x] = (bf16_t)s;
        if (threadIdx.x == 0) lse[bh] = l;
    }
}

template <int HI, bool DROP>
__global__ __launch_bounds__(256) void AV_KERNEL(cls_bwd_kernel)(const bf16_t *__restrict__ qkv, const bf16_t *__restrict__ o_cls,
                                                        const bf16_t *__restrict__ do_cls, const float *__restrict__ lse,
                                                        bf16_t *__restrict__ dqkv, bf16_t *__restrict__ dq_cls, AV_LENGTHS int N, int h,
                                                        float scale, uint64_t seed, uint32_t thresh, float inv_keep) {
    AV_ROW_BASE
    constexpr int DH = 64 * HI, G = 8 * HI, SLOTS = 256 / G;
    __shared__ float qred[SLOTS][DH + 1];
    const int bh = blockIdx.x, b = bh / h, head = bh % h;
    const int n = UN ? N : n_tok[b];
    const int g = threadIdx.x % G, slot = threadIdx.x / G;
    const int64_t dm = (int64_t)h * DH, ld = 3 * dm;
    if constexpr (!UN && !PK) {   // rows >= n: dK = dV = 0
        av_zero_rows<DH>(dqkv + (int64_t)b * N * ld + dm + head * DH, ld, n, N);
        av_zero_rows<DH>(dqkv + (int64_t)b * N * ld + 2 * dm + head * DH, ld, n, N);
    }
    const int64_t roff = PK ? (int64_t)tok_off[b] * ld + head * DH + g * 8 : (int64_t)b * N * ld + head * DH + g * 8;
    const bf16_t *rec = qkv + roff;
    bf16_t *drec = dqkv + roff;
    const Vec16<bf16_t> q = ld16(rec), dO = ld16(do_cls + (int64_t)b * dm + head * DH + g * 8), O = ld16(o_cls + (int64_t)b * dm + head * DH + g * 8);
    float D = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) D = fmaf(dO.get(t), O.get(t), D);
    D = avc_group_sum<HI>(D);
    const float l = lse[bh];
    const uint32_t smix = seed_mix(seed), quad0 = (uint32_t)bh * (uint32_t)N * (uint32_t)((N + 3) >> 2);
    float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = slot; k < n; k += SLOTS) {
        const Vec16<bf16_t> kv = ld16(rec + (int64_t)k * ld + dm), vv = ld16(rec + (int64_t)k * ld + 2 * dm);
        float s = 0.f, dp = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t) { s = fmaf(q.get(t), kv.get(t), s); dp = fmaf(dO.get(t), vv.get(t), dp); }
        s = avc_group_sum<HI>(s);
        dp = avc_group_sum<HI>(dp);
        const float p = __expf(s * scale - l), mlt = avc_mult<DROP>(smix, quad0, k, thresh, inv_keep);
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
    if (threadIdx.x < DH) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < SLOTS; ++j) s += qred[j][threadIdx.x];
        dq_cls[(int64_t)b * dm + head * DH + threadIdx.x] = (bf16_t)(s * scale);
    }
}

#undef AV_KERNEL
#undef AV_LENGTHS
#undef AV_ROW_BASE
