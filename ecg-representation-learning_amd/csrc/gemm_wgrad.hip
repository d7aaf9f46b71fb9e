// Weight-gradient products dW = dY^T . X for the Linear layers (C = A^T . B, both operands k-major: A[K, M], B[K, N] row-major with
// K = token rows): 256 x 256 x 64 block tile, 4 waves (2 x 2, wave tile 128 x 128), v_mfma_f32_32x32x16_bf16, split-K over the token
// rows with f32 slabs + a deterministic reduce.
//
// gemm_wgrad_kernel_4w: one (K-slice, tile) item per block; operands stream HBM -> LDS by LDS-DMA (`buffer_load ... lds`, no VGPR
// staging): A tiles ([64 k][256 m], 32 KiB) two K-tiles ahead in a 3-slot ring, B tiles one ahead in 2 slots (5 x 32 KiB = all of
// LDS); ONE counted vmcnt and ONE workgroup barrier per K-tile.  K-slices are pinned to XCDs (slice counts that are multiples of 8) or
// laid out XCD-contiguously, so a slice's operand rows live in one L2.
// LDS image of a k-major operand: [64 k][256 mn] (512-B rows), 16-B chunk ^= (k&3)<<2 (applied to the per-lane SOURCE address: the
// DMA destination is wave-uniform base + lane*16) -- the 4 k-rows of one transposed half-wave read land on the 4 distinct 64-B
// quarters of the bank row.  Rows beyond a slice's end fall outside the buffer descriptor and read as zero.
// The transposed reads are inline asm: with an LDS-DMA in flight hipcc's waitcnt pass drains vmcnt(0) in front of the builtin.
// Also here: the column-sum reducer shared with gemm_nt.hip's EPI_COLSUM.
#include "gemm_plan.h"
#include <algorithm>
#include <type_traits>
#include <utility>

namespace {

constexpr int BM = GEMM_WGRAD_TILE, BN = GEMM_WGRAD_TILE, BK = GEMM_BK;
constexpr int TILE_BYTES = 32768;
constexpr int CS_LD = 68, CS_WAVE_BYTES = 64 * CS_LD * 4;  // 17408: per-wave epilogue patch (64 rows x 64 f32 + pad)
constexpr int LDS_BYTES = 163840;                          // all of LDS: 3 A + 2 B tiles; the epilogue patches need 139264

typedef __attribute__((address_space(3))) void *lptr_t;

__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7, j = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

struct SplitK2 {
    int splits, k_per_split;
    float *slabs;
};

// Finish one 8-column piece of an output row: split-K slab store, or alpha / bias / GELU (+aux) / dropout / GELU' / residual /
// accumulate, then a 16-B (bf16) or 2 x 16-B (f32) store.  `cs` accumulates the column sums of what is stored (EPI_COLSUM).
template <typename TO>
__device__ __forceinline__ void epi_row8(const f32x4 c0, const f32x4 c1, int64_t m, int n, const ecgvit_gemm_desc &d,
                                         const EpiParams &e, const SplitK2 &sk, int split, float (&cs)[8]) {
    const int M = d.M, N = d.N;
    if (m >= M || n >= N) return;
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = c0[k]; v[4 + k] = c1[k]; }
    if (sk.splits > 1) {
        float *o = sk.slabs + ((int64_t)split * M + m) * N + n;
        *reinterpret_cast<f32x4 *>(o) = c0;
        *reinterpret_cast<f32x4 *>(o + 4) = c1;
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] *= e.alpha;
    if (e.flags & ECGVIT_EPI_BIAS) {
        const f32x4 b0 = *reinterpret_cast<const f32x4 *>(e.bias + n), b1 = *reinterpret_cast<const f32x4 *>(e.bias + n + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] += b0[k]; v[4 + k] += b1[k]; }
    }
    if constexpr (sizeof(TO) == 2) {
        float mult[8];
        const bool drop = e.flags & ECGVIT_EPI_DROPOUT;
        if (drop) dropout_mask8(e.seed, (uint32_t)m * (uint32_t)e.N + (uint32_t)n, e.drop_thresh, e.inv_keep, mult);
        if (e.flags & ECGVIT_EPI_GELU) {
            Vec16<bf16_t> sav;
            if (e.flags & ECGVIT_EPI_GELU_GRAD_AUX) {   // aux = gelu'(v) * dropout multiplier: all the backward of this site needs
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float dy;
                    gelu_fast_both(v[k], v[k], dy);
                    sav.set(k, drop ? dy * mult[k] : dy);
                }
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) sav.set(k, v[k]);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = gelu_fast(sav.get(k));
            }
            st16(reinterpret_cast<bf16_t *>(e.aux) + m * e.ldaux + n, sav);
        }
        if (drop) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= mult[k];
        }
        if (e.flags & ECGVIT_EPI_GELU_BWD) {
            const Vec16<bf16_t> pre = ld16(reinterpret_cast<const bf16_t *>(e.aux) + m * e.ldaux + n);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= gelu_fast_grad(pre.get(k));
        }
        if (e.flags & ECGVIT_EPI_MUL_AUX) {
            const Vec16<bf16_t> a = ld16(reinterpret_cast<const bf16_t *>(e.aux) + m * e.ldaux + n);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= a.get(k);
        }
        if (e.flags & ECGVIT_EPI_RESIDUAL) {
            const Vec16<bf16_t> res = ld16(reinterpret_cast<const bf16_t *>(e.residual) + m * e.ldr + n);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] += res.get(k);
        }
        bf16_t *o = reinterpret_cast<bf16_t *>(d.C) + m * d.ldc + n;
        if (e.flags & ECGVIT_EPI_ACCUM) {
            const Vec16<bf16_t> old = ld16(o);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] += old.get(k);
        }
        Vec16<bf16_t> out;
#pragma unroll
        for (int k = 0; k < 8; ++k) out.set(k, v[k]);
        st16(o, out);
#pragma unroll
        for (int k = 0; k < 8; ++k) cs[k] += out.get(k);
    } else {
        float *o = reinterpret_cast<float *>(d.C) + m * d.ldc + n;
        if (e.flags & ECGVIT_EPI_ACCUM) {
            const f32x4 o0 = *reinterpret_cast<const f32x4 *>(o), o1 = *reinterpret_cast<const f32x4 *>(o + 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) { v[k] += o0[k]; v[4 + k] += o1[k]; }
        }
        f32x4 w0, w1;
#pragma unroll
        for (int k = 0; k < 4; ++k) { w0[k] = v[k]; w1[k] = v[4 + k]; }
        *reinterpret_cast<f32x4 *>(o) = w0;
        *reinterpret_cast<f32x4 *>(o + 4) = w1;
    }
}

__device__ __forceinline__ void epi_colsum_flush(float (&cs)[8], const ecgvit_gemm_desc &d, const EpiParams &e, int m0, int n, int wm,
                                                 int lane) {
    if (!(e.flags & ECGVIT_EPI_COLSUM)) return;
    // lanes with equal (lane & 7) hold the same 8 columns: fold the 8 row groups, then one partial row per (tile row, wm)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        cs[k] += __shfl_xor(cs[k], 8, 64);
        cs[k] += __shfl_xor(cs[k], 16, 64);
        cs[k] += __shfl_xor(cs[k], 32, 64);
    }
    if (lane < 8 && n < d.N) {
        float *pr = reinterpret_cast<float *>(d.workspace) + ((int64_t)(m0 / BM) * 2 + wm) * d.N + n;
#pragma unroll
        for (int k = 0; k < 8; ++k) pr[k] = cs[k];
    }
}

// Drain one wave's 128 x 64 accumulator block through its private LDS patch (two 64-row passes) and store 128-B row segments.
template <typename TO>
__device__ __forceinline__ void epilogue_store(f32x16 (&acc)[4][2], char *smem, const ecgvit_gemm_desc &d, const EpiParams &e,
                                               const SplitK2 &sk, int split, int m0, int n0, int wave, int lane) {
    const int wm = wave >> 2, wn = wave & 3;
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float *Cs = reinterpret_cast<float *>(smem + wave * CS_WAVE_BYTES);
    const int lr = lane & 31, lh = lane >> 5;
    const int cc = (lane & 7) * 8;
    const int n = n0 + wn * 64 + cc;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Cs[(ii * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * CS_LD + j * 32 + lr] = acc[hh * 2 + ii][j][r];
        // same-wave LDS ops execute in order: the reads below see the writes above
#pragma unroll 1
        for (int p = 0; p < 8; ++p) {
            const int rr = p * 8 + (lane >> 3);
            const f32x4 c0 = *reinterpret_cast<const f32x4 *>(&Cs[rr * CS_LD + cc]);
            const f32x4 c1 = *reinterpret_cast<const f32x4 *>(&Cs[rr * CS_LD + cc + 4]);
            epi_row8<TO>(c0, c1, (int64_t)m0 + wm * 128 + hh * 64 + rr, n, d, e, sk, split, cs);
        }
    }
    epi_colsum_flush(cs, d, e, m0, n, wm, lane);
}

// ------------------------------------------------------------------------------------------------------------------
// gemm_wgrad_kernel_4w: FOUR waves -- one per SIMD, each owning a 128 x 128 block of the tile in 256 accumulator registers (4 x 4 tiles of
// v_mfma_f32_32x32x16_bf16).  A 16-deep k-step is ONE instruction stream of 16 MFMAs (512 cycles) with the next k-step's 16 transposed
// fragment reads and four DMA pieces placed between them in a fixed order.  Against the eight-wave kernel it replaced (2 x 4 waves of
// 128 x 64, four 16-deep phases per K-tile, waves 4-7 one barrier behind waves 0-3): 64 instead of 96 fragment reads per k-step and CU,
// ONE workgroup barrier per K-tile instead of eight (it stands between k-steps 2 and 3: behind it K-tile kt+1 is visible and nobody reads
// K-tile kt from LDS any more, so B(kt+2) and A(kt+3) may go out), and bit-identical results (same MFMA, same K order per accumulator).
template <int... X, typename F>
__device__ __forceinline__ void w4_static_for_impl(std::integer_sequence<int, X...>, F &&f) { (f(std::integral_constant<int, X>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void w4_static_for(F &&f) { w4_static_for_impl(std::make_integer_sequence<int, N>{}, f); }

template <typename TO>
__global__ __launch_bounds__(256, 1) void gemm_wgrad_kernel_4w(ecgvit_gemm_desc d, EpiParams e, SplitK2 sk, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
    const int ntile = tiles_m * tiles_n;
    int split, tid;
    if (sk.splits > 1 && (sk.splits & 7) == 0) {
        const int r = sk.splits >> 3, x = blockIdx.x & 7, q = blockIdx.x >> 3;
        split = x + 8 * (q % r);
        tid = q / r;
    } else if (sk.splits > 1) {
        const int gid = xcd_remap(blockIdx.x, ntile * sk.splits);
        split = gid / ntile;
        tid = gid - split * ntile;
    } else {
        split = 0;
        tid = xcd_remap(blockIdx.x, ntile);
    }
    const int tm = tid / tiles_n, tn = tid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = split * sk.k_per_split;
    const int kend = min(d.K, kbeg + sk.k_per_split);
    const int nk = (kend - kbeg + BK - 1) / BK;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int lda2 = (int)d.lda * 2, ldb2 = (int)d.ldb * 2;

    // DMA: eight 1-KiB pieces of a 32-KiB tile per wave; piece 8*wave + i = k-rows 16*wave + 2*i + {0, 1}: pieces i and i + 4 share the
    // per-lane offset (same row swizzle), the 8 rows between them go into the scalar offset.  Rows >= kend read as zero (descriptor);
    // pieces of K-tiles past the slice's end are sent through an EMPTY descriptor instead of around a branch.
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.A), 0, (uint32_t)((int64_t)kend * lda2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.B), 0, (uint32_t)((int64_t)kend * ldb2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.A), 0, 0u, 0x00020000);
    int voA[4], voB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kr = 16 * wave + 2 * i + (lane >> 5);
        const int c = (lane & 31) ^ ((kr & 3) << 2);
        voA[i] = kr * lda2 + (m0 + c * 8) * 2;
        voB[i] = kr * ldb2 + (n0 + c * 8) * 2;
    }
#define W4_PIECE(RS, VO, LD2, SLOT, K0, I) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lptr_t)(smem + (SLOT) * TILE_BYTES + (8 * wave + (I)) * 1024), 16, VO[(I) & 3], (K0) * (LD2) + ((I) >> 2) * 8 * (LD2), 0, 0)
    // fragment reads: lane (g = lane >> 4, i = lane & 15) of the 32 x 16 fragment of 32-column tile t, k-step ks reads 8 bytes at
    // k = 16 ks + 8 (g >> 1) + (i >> 2) [and k + 4], columns 32 t + 16 (g & 1) + 4 (i & 3) ..: per lane one offset per tile t (the image's row
    // swizzle folds into the tile index), k-step and the k + 4 half are immediates
    const uint32_t sm = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    uint32_t foA[4], foB[4];
    {
        const int g = lane >> 4, i = lane & 15;
        const int base = ((g >> 1) * 8 + (i >> 2)) * 512 + ((g & 1) * 16 + (i & 3) * 4) * 2, sw = (i >> 2) & 3;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            foA[t] = sm + base + wm * 256 + ((t ^ sw) << 6);
            foB[t] = sm + base + wn * 256 + ((t ^ sw) << 6);
        }
    }
    // two fragment buffers (this k-step's and the next one's): lo = k .. k+3 half, hi = k+4 .. half of a lane's 8 k
    bf16x4 alo[2][4], ahi[2][4], blo[2][4], bhi[2][4];
#define W4_READ(DST_LO, DST_HI, ADDR, KS)                                                                                    \
    do {                                                                                                                     \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(DST_LO) : "v"(ADDR), "n"((KS) * 8192) : "memory");         \
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(DST_HI) : "v"(ADDR), "n"((KS) * 8192 + 2048) : "memory");  \
    } while (0)
#define W4_FENCE() __builtin_amdgcn_sched_barrier(0)

    f32x16 acc[2][4][2];   // [column half][row tile][column tile of the half]: the epilogue drains two 128 x 64 halves
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.f;

    // prologue: A(0), B(0), A(1); behind the barrier the first half of B(1) and the first k-step's fragments
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsA, voA, lda2, 0, kbeg, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsB, voB, ldb2, 3, kbeg, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsA, voA, lda2, 1, kbeg + BK, i);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 4; ++i) W4_PIECE(rsB, voB, ldb2, 4, kbeg + BK, i);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const uint32_t ab = foA[t], bb = foB[t] + 3 * TILE_BYTES;
        W4_READ(blo[0][t], bhi[0][t], bb, 0);
        W4_READ(alo[0][t], ahi[0][t], ab, 0);
    }

    int ga = 0, gb = 0;
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
        const int ga1 = ga == 2 ? 0 : ga + 1, ga2 = ga == 0 ? 2 : ga - 1, gb1 = gb ^ 1;
        const int kB1 = kbeg + (kt + 1) * BK, kA2 = kbeg + (kt + 2) * BK;
        const bool ok1 = kt + 1 < nk, ok2 = kt + 2 < nk;
        const __amdgpu_buffer_rsrc_t rB1 = ok1 ? rsB : rs0, rA2 = ok2 ? rsA : rs0, rB2 = ok2 ? rsB : rs0;
        // one k-step: 16 MFMAs from buffer CUR; the next k-step's 16 reads into buffer CUR ^ 1 (tile bases NA / NB, k-step NKS) behind
        // MFMAs 0-11 (two each behind the first four: all B fragments, then one A half per MFMA) and four DMA pieces behind MFMAs 2, 6, 10, 14
#define W4_KSTEP(CUR, NA, NB, NKS, RS, VO, LD2, SLOT, K0, P0)                                                                \
    do {                                                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                   \
        W4_FENCE();                                                                                                          \
        w4_static_for<16>([&](auto xc_) __attribute__((always_inline)) {                                                     \
            constexpr int x_ = decltype(xc_)::value, i_ = x_ >> 2, j_ = x_ & 3;                                              \
            {                                                                                                                \
                const u32x2 al_ = __builtin_bit_cast(u32x2, alo[CUR][i_]), ah_ = __builtin_bit_cast(u32x2, ahi[CUR][i_]);    \
                const u32x2 bl_ = __builtin_bit_cast(u32x2, blo[CUR][j_]), bh_ = __builtin_bit_cast(u32x2, bhi[CUR][j_]);    \
                const u32x4 au_ = {al_[0], al_[1], ah_[0], ah_[1]}, bu_ = {bl_[0], bl_[1], bh_[0], bh_[1]};                   \
                acc[j_ >> 1][i_][j_ & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, au_), __builtin_bit_cast(bf16x8, bu_), \
                                                                                  acc[j_ >> 1][i_][j_ & 1], 0, 0, 0);        \
            }                                                                                                                \
            W4_FENCE();                                                                                                      \
            if constexpr (x_ < 4) {                                                                                          \
                W4_READ(blo[(CUR) ^ 1][x_], bhi[(CUR) ^ 1][x_], (NB)[x_], NKS);                                              \
                W4_FENCE();                                                                                                  \
            } else if constexpr (x_ < 12) {                                                                                  \
                constexpr int t_ = (x_ - 4) >> 1;                                                                            \
                if constexpr ((x_ & 1) == 0) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(alo[(CUR) ^ 1][t_]) : "v"((NA)[t_]), "n"((NKS) * 8192) : "memory"); \
                else asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(ahi[(CUR) ^ 1][t_]) : "v"((NA)[t_]), "n"((NKS) * 8192 + 2048) : "memory"); \
                W4_FENCE();                                                                                                  \
            }                                                                                                                \
            if constexpr ((x_ & 3) == 2) {                                                                                   \
                W4_PIECE(RS, VO, LD2, SLOT, K0, (P0) + (x_ >> 2));                                                           \
                W4_FENCE();                                                                                                  \
            }                                                                                                                \
        });                                                                                                                  \
    } while (0)
        uint32_t ca[4], cb[4], na[4], nb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ca[t] = foA[t] + ga * TILE_BYTES; cb[t] = foB[t] + (3 + gb) * TILE_BYTES;
            na[t] = foA[t] + ga1 * TILE_BYTES; nb[t] = foB[t] + (3 + gb1) * TILE_BYTES;
        }
        W4_KSTEP(0, ca, cb, 1, rB1, voB, ldb2, 3 + gb1, kB1, 4);    // second half of B(kt+1)
        W4_KSTEP(1, ca, cb, 2, rA2, voA, lda2, ga2, kA2, 0);        // A(kt+2)
        W4_KSTEP(0, ca, cb, 3, rA2, voA, lda2, ga2, kA2, 4);
        // the K-tile's one counted wait and one barrier: everything but A(kt+2) has landed; this wave's reads of K-tile kt have retired
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        W4_FENCE();
        __builtin_amdgcn_s_barrier();
        W4_FENCE();
        W4_KSTEP(1, na, nb, 0, rB2, voB, ldb2, 3 + gb, kB1 + BK, 0);   // first half of B(kt+2), into the slot of B(kt); reads of K-tile kt+1
        ga = ga1; gb = gb1;
    }
#undef W4_KSTEP
#undef W4_READ
#undef W4_PIECE
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    W4_FENCE();
    __builtin_amdgcn_s_barrier();
#undef W4_FENCE
    // the epilogue's per-wave LDS patches: one per (wave, column half) -- eight in all, as with eight waves
    epilogue_store<TO>(acc[0], smem, d, e, sk, split, m0, n0, 4 * wm + 2 * wn, lane);
    epilogue_store<TO>(acc[1], smem, d, e, sk, split, m0, n0, 4 * wm + 2 * wn + 1, lane);
}


// ------------------------------------------------------------------------------------------------------------------
// The same kernel on 8-BIT operands (fp8_linear; BASELINE.json configs[4]): dW = dY8^T . X8 with dY8 in e5m2 (or e4m3) and X8 in e4m3,
// both k-major ([token rows][features], one byte per element -- the copies the forward / input-gradient products already own), on the
// block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (twice the bf16 MFMA rate).  A K-tile is 128 token rows deep in
// the same 32-KiB tile ([128 k][256 mn] bytes, 256-B rows), i.e. twice the K per byte that crosses the CU's memory path.
// Fragments come from `ds_read_b64_tr_b8` (probed on the device, tools/probe_tr8.hip): in a 16-lane group source lane s supplies the
// 8 bytes at ITS address and result lane i receives byte (i & 7) of source lanes 2j + (i >> 3), j = 0..7 -- with source lane s pointing
// at k-row s >> 1, bytes 8 (s & 1) .. +7 of a 16-byte column chunk, lane i ends up with 8 consecutive k of column i.  Four such reads
// (k = 32 hb + 8 t + j) are the 32 operand bytes of one lane (row lane & 31, k-half hb = lane >> 5); A and B use the same k order.
// Image swizzle (on the per-lane SOURCE address of the DMA): 16-B chunk ^= (k & 7) << 1 -- the 8 k-rows x 2 column chunks a 32-lane
// read cycle touches land on 16 distinct 16-B slots of the 256-B bank row.
typedef int i32x8_t __attribute__((ext_vector_type(8)));

// per-lane byte offset (inside a tile image) of the lane's first transposed read for a 32-column block starting at column mn_base (a
// multiple of 32); read t of k-step ks adds 16384 ks + 2048 t
__device__ __forceinline__ uint32_t frag8_lane_off(int mn_base, int lane) {
    const int s = lane & 15, j = s >> 1;
    const int chunk = (mn_base >> 4) + ((lane >> 4) & 1);
    return (uint32_t)((32 * (lane >> 5) + j) * 256 + ((chunk ^ (j << 1)) << 4) + 8 * (s & 1));
}
// gemm_wgrad8_kernel_4w: the 8-bit weight-gradient kernel with FOUR waves (one per SIMD, 128 x 128 per wave in 256 accumulator registers):
// a 64-deep k-step is one instruction stream of 16 MFMAs (v_mfma_scale_f32_32x32x64_f8f6f4, 64 cycles each) with the next k-step's 32
// transposed reads and eight DMA pieces between them; one barrier per 128-deep K-tile, between its two k-steps.
template <int AFMT>
__global__ __launch_bounds__(256, 1) void gemm_wgrad8_kernel_4w(ecgvit_gemm_desc d, EpiParams e, SplitK2 sk, int tiles_m, int tiles_n) {
    __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
    constexpr int BK8 = 128;
    const int ntile = tiles_m * tiles_n;
    int split, tid;
    if (sk.splits > 1 && (sk.splits & 7) == 0) {
        const int r = sk.splits >> 3, x = blockIdx.x & 7, q = blockIdx.x >> 3;
        split = x + 8 * (q % r);
        tid = q / r;
    } else if (sk.splits > 1) {
        const int gid = xcd_remap(blockIdx.x, ntile * sk.splits);
        split = gid / ntile;
        tid = gid - split * ntile;
    } else {
        split = 0;
        tid = xcd_remap(blockIdx.x, ntile);
    }
    const int tm = tid / tiles_n, tn = tid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    const int kbeg = split * sk.k_per_split;
    const int kend = min(d.K, kbeg + sk.k_per_split);
    const int nk = (kend - kbeg + BK8 - 1) / BK8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int lda1 = (int)d.lda, ldb1 = (int)d.ldb;   // byte pitches
    if (d.scale_a) e.alpha *= *d.scale_a;
    if (d.scale_b) e.alpha *= *d.scale_b;

    // DMA: eight 1-KiB pieces (4 k-rows x 256 B) of a 32-KiB tile per wave: piece 8*wave + i = k-rows 32*wave + 4*i + (lane >> 4); pieces i and
    // i + 4 share the per-lane offset (same swizzle: 16 rows apart), the 16 rows go into the scalar offset
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.A), 0, (uint32_t)((int64_t)kend * lda1), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.B), 0, (uint32_t)((int64_t)kend * ldb1), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(d.A), 0, 0u, 0x00020000);
    int voA[4], voB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kr = 32 * wave + 4 * i + (lane >> 4);
        const int c = (lane & 15) ^ ((kr & 7) << 1);
        voA[i] = kr * lda1 + m0 + c * 16;
        voB[i] = kr * ldb1 + n0 + c * 16;
    }
#define W4_PIECE(RS, VO, LD1, SLOT, K0, I) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lptr_t)(smem + (SLOT) * TILE_BYTES + (8 * wave + (I)) * 1024), 16, VO[(I) & 3], (K0) * (LD1) + ((I) >> 2) * 16 * (LD1), 0, 0)
    const uint32_t sm = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)smem;
    uint32_t foA[4], foB[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        foA[t] = sm + frag8_lane_off(wm * 128 + t * 32, lane);
        foB[t] = sm + frag8_lane_off(wn * 128 + t * 32, lane);
    }
    // two fragment buffers; fragment f: 0-3 = B column blocks, 4-7 = A row blocks; four 8-byte transposed reads each
    u32x2 fr[2][8][4];
#define W4_FENCE() __builtin_amdgcn_sched_barrier(0)
#define W4_READ8(BUF, F, T, ADDR, KS) \
    asm volatile("ds_read_b64_tr_b8 %0, %1 offset:%2" : "=v"(fr[BUF][F][T]) : "v"(ADDR), "n"((KS) * 16384 + 2048 * (T)) : "memory")

    f32x16 acc[2][4][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][i][j][r] = 0.f;

    // prologue: A(0), B(0), A(1); behind the barrier B(1) and the first k-step's fragments
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsA, voA, lda1, 0, kbeg, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsB, voB, ldb1, 3, kbeg, i);
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsA, voA, lda1, 1, kbeg + BK8, i);
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int i = 0; i < 8; ++i) W4_PIECE(rsB, voB, ldb1, 4, kbeg + BK8, i);
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const uint32_t ad = f < 4 ? foB[f & 3] + 3 * TILE_BYTES : foA[f & 3];
#pragma unroll
        for (int t = 0; t < 4; ++t) W4_READ8(0, f, t, ad, 0);
    }

    int ga = 0, gb = 0;
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
        const int ga1 = ga == 2 ? 0 : ga + 1, ga2 = ga == 0 ? 2 : ga - 1, gb1 = gb ^ 1;
        const int kn = kbeg + (kt + 2) * BK8;
        const bool ok2 = kt + 2 < nk;
        const __amdgpu_buffer_rsrc_t rA2 = ok2 ? rsA : rs0, rB2 = ok2 ? rsB : rs0;
        uint32_t ca[4], cb[4], na[4], nb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ca[t] = foA[t] + ga * TILE_BYTES; cb[t] = foB[t] + (3 + gb) * TILE_BYTES;
            na[t] = foA[t] + ga1 * TILE_BYTES; nb[t] = foB[t] + (3 + gb1) * TILE_BYTES;
        }
        // one k-step: 16 MFMAs from buffer CUR; the next k-step's 32 reads into CUR ^ 1 behind MFMAs 0-11 (three each behind the first
        // eight, two behind the next four; B fragments first) and eight DMA pieces, one behind every other MFMA
#define W8_KSTEP(CUR, NA, NB, NKS, RS, VO, LD1, SLOT)                                                                         \
    do {                                                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                   \
        W4_FENCE();                                                                                                          \
        w4_static_for<16>([&](auto xc_) __attribute__((always_inline)) {                                                     \
            constexpr int x_ = decltype(xc_)::value, i_ = x_ >> 2, j_ = x_ & 3;                                              \
            {                                                                                                                \
                const i32x8_t a_ = {(int)fr[CUR][4 + i_][0][0], (int)fr[CUR][4 + i_][0][1], (int)fr[CUR][4 + i_][1][0], (int)fr[CUR][4 + i_][1][1], \
                                    (int)fr[CUR][4 + i_][2][0], (int)fr[CUR][4 + i_][2][1], (int)fr[CUR][4 + i_][3][0], (int)fr[CUR][4 + i_][3][1]}; \
                const i32x8_t b_ = {(int)fr[CUR][j_][0][0], (int)fr[CUR][j_][0][1], (int)fr[CUR][j_][1][0], (int)fr[CUR][j_][1][1],   \
                                    (int)fr[CUR][j_][2][0], (int)fr[CUR][j_][2][1], (int)fr[CUR][j_][3][0], (int)fr[CUR][j_][3][1]};   \
                acc[j_ >> 1][i_][j_ & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a_, b_, acc[j_ >> 1][i_][j_ & 1], AFMT, 0, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F); \
            }                                                                                                                \
            W4_FENCE();                                                                                                      \
            constexpr int r0_ = x_ < 8 ? 3 * x_ : 24 + 2 * (x_ - 8), nr_ = x_ < 8 ? 3 : x_ < 12 ? 2 : 0;                     \
            if constexpr (nr_ > 0) { W4_READ8((CUR) ^ 1, (r0_ >> 2), (r0_ & 3), ((r0_ >> 2) < 4 ? (NB)[(r0_ >> 2) & 3] : (NA)[(r0_ >> 2) & 3]), NKS); } \
            if constexpr (nr_ > 1) { W4_READ8((CUR) ^ 1, ((r0_ + 1) >> 2), ((r0_ + 1) & 3), (((r0_ + 1) >> 2) < 4 ? (NB)[((r0_ + 1) >> 2) & 3] : (NA)[((r0_ + 1) >> 2) & 3]), NKS); } \
            if constexpr (nr_ > 2) { W4_READ8((CUR) ^ 1, ((r0_ + 2) >> 2), ((r0_ + 2) & 3), (((r0_ + 2) >> 2) < 4 ? (NB)[((r0_ + 2) >> 2) & 3] : (NA)[((r0_ + 2) >> 2) & 3]), NKS); } \
            if constexpr (nr_ > 0) W4_FENCE();                                                                               \
            if constexpr ((x_ & 1) == 1) {                                                                                   \
                W4_PIECE(RS, VO, LD1, SLOT, kn, x_ >> 1);                                                                    \
                W4_FENCE();                                                                                                  \
            }                                                                                                                \
        });                                                                                                                  \
    } while (0)
        W8_KSTEP(0, ca, cb, 1, rA2, voA, lda1, ga2);          // A(kt+2) goes out
        asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        W4_FENCE();
        __builtin_amdgcn_s_barrier();
        W4_FENCE();
        W8_KSTEP(1, na, nb, 0, rB2, voB, ldb1, 3 + gb);       // B(kt+2) into the slot of B(kt); reads of K-tile kt+1
        ga = ga1; gb = gb1;
    }
#undef W8_KSTEP
#undef W4_READ8
#undef W4_PIECE
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    W4_FENCE();
    __builtin_amdgcn_s_barrier();
#undef W4_FENCE
    epilogue_store<float>(acc[0], smem, d, e, sk, split, m0, n0, 4 * wm + 2 * wn, lane);
    epilogue_store<float>(acc[1], smem, d, e, sk, split, m0, n0, 4 * wm + 2 * wn + 1, lane);
}

template <typename TO>
__global__ __launch_bounds__(256) void splitk_reduce2_kernel(const float *__restrict__ slabs, int splits, int64_t MN, int N,
                                                             TO *__restrict__ C, int64_t ldc, EpiParams e,
                                                             const float *__restrict__ scale_a = nullptr, const float *__restrict__ scale_b = nullptr) {
    if (scale_a) e.alpha *= *scale_a;   // per-tensor scales of 8-bit operands
    if (scale_b) e.alpha *= *scale_b;
    const int64_t nv = MN / 4;
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        f32x4 s = *reinterpret_cast<const f32x4 *>(slabs + i * 4);
        for (int k = 1; k < splits; ++k) s += *reinterpret_cast<const f32x4 *>(slabs + (int64_t)k * MN + i * 4);
        const int64_t m = (i * 4) / N;
        const int n = (int)((i * 4) - m * N);
        TO *o = C + m * ldc + n;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v = s[k] * e.alpha;
            if (e.flags & ECGVIT_EPI_BIAS) v += e.bias[n + k];
            if (e.flags & ECGVIT_EPI_ACCUM) v += to_f32<TO>(o[k]);
            o[k] = from_f32<TO>(v);
        }
    }
}

__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float *__restrict__ partial, int nparts, int N, float *__restrict__ out) {
    // 64 columns x 16 row slices per block (N/64 blocks only: the parallelism comes from inside the block); deterministic tree
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (c < N) {
        int p = slice;
        for (; p + 48 < nparts; p += 64) {
            s0 += partial[(int64_t)p * N + c];
            s1 += partial[(int64_t)(p + 16) * N + c];
            s2 += partial[(int64_t)(p + 32) * N + c];
            s3 += partial[(int64_t)(p + 48) * N + c];
        }
        for (; p < nparts; p += 16) s0 += partial[(int64_t)p * N + c];
    }
    red[slice][lane] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (slice == 0 && c < N) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 16; r += 4) { t[0] += red[r][lane]; t[1] += red[r + 1][lane]; t[2] += red[r + 2][lane]; t[3] += red[r + 3][lane]; }
        out[c] = (t[0] + t[1]) + (t[2] + t[3]);
    }
}

}  // namespace

void ecgvit_colsum_reduce_launch(const float *partial, int nparts, int N, float *out, hipStream_t s) {
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3((N + 63) / 64), dim3(1024), 0, s, partial, nparts, N, out);
}

int gemm_wgrad_launch(const GemmPlan &p, const ecgvit_gemm_desc *d, hipStream_t s) {
    SplitK2 sk;
    sk.splits = p.splits;
    sk.k_per_split = p.k_per_split;
    sk.slabs = p.splits > 1 ? reinterpret_cast<float *>(d->workspace) : nullptr;
    const EpiParams e = make_epi(d, p.mask_row_pitch);
    const bool f8 = p.body == GemmBody::WGRAD8;
    if (f8) {
        if (d->dtype == ECGVIT_BF8_E5M2) hipLaunchKernelGGL(gemm_wgrad8_kernel_4w<1>, p.grid, dim3(256), 0, s, *d, e, sk, p.tiles_m, p.tiles_n);
        else hipLaunchKernelGGL(gemm_wgrad8_kernel_4w<0>, p.grid, dim3(256), 0, s, *d, e, sk, p.tiles_m, p.tiles_n);
    } else {
        if (d->out_dtype == ECGVIT_BF16) hipLaunchKernelGGL(gemm_wgrad_kernel_4w<bf16_t>, p.grid, dim3(256), 0, s, *d, e, sk, p.tiles_m, p.tiles_n);
        else hipLaunchKernelGGL(gemm_wgrad_kernel_4w<float>, p.grid, dim3(256), 0, s, *d, e, sk, p.tiles_m, p.tiles_n);
    }
    ECGVIT_CHECK_LAUNCH();
    if (sk.splits > 1) {
        const int64_t MN = (int64_t)d->M * d->N;
        const int g = (int)std::min<int64_t>((MN / 4 + 255) / 256, 2048);
        if (d->out_dtype == ECGVIT_BF16) hipLaunchKernelGGL(splitk_reduce2_kernel<bf16_t>, dim3(g), dim3(256), 0, s, sk.slabs, sk.splits, MN, d->N, (bf16_t *)d->C, d->ldc, e);
        else hipLaunchKernelGGL(splitk_reduce2_kernel<float>, dim3(g), dim3(256), 0, s, sk.slabs, sk.splits, MN, d->N, (float *)d->C, d->ldc, e,
                                f8 ? d->scale_a : nullptr, f8 ? d->scale_b : nullptr);
        ECGVIT_CHECK_LAUNCH();
    }
    return ECGVIT_OK;
}
