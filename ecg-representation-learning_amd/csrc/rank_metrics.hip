// Rank-based AUROC and bootstrap replicates (beside metrics.hip): one stable radix sort of every class column, then a
// weighted prefix sum over the sorted order per replicate -- O(n K) a replicate where the all-pairs kernel costs O(n^2 K).  Contract, key,
// packing, generator and limits: include/ecgvit_hip_rank.h.  Everything the device produces is an exact integer; integer atomics only (LDS
// histograms, the multiplicity counts), which are order-free; no kernel waits for another workgroup.
#include "metrics_common.h"
#include "../../include/ecgvit_hip_rank.h"

#define RANK_TILE ECGVIT_RANK_TILE
#define RANK_THREADS 256
#define RANK_WAVE_ROWS (RANK_TILE / 4)          // a wave's quarter of a tile
#define RANK_STEPS (RANK_WAVE_ROWS / WAVE)      // 64-row steps of a wave
#define RANK_NAN_KEY 0xFFFFFFFFu
static_assert(RANK_TILE % (4 * WAVE) == 0, "tile of whole wave steps");

// ---- keys ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rank_key(float p) {
    if (p != p) return RANK_NAN_KEY;
    if (p == 0.f) p = 0.f;   // -0 and +0: one key
    const uint32_t b = __float_as_uint(p);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// (n, K) scores with row pitch ld -> (K, n) keys: a 64 x 64 tile through LDS, so that the read runs along the classes and the write along the records
__global__ __launch_bounds__(RANK_THREADS) void rank_keys_kernel(const float *__restrict__ scores, int64_t ld, int64_t n, int K, int from_logits,
                                                                 uint32_t *__restrict__ keys) {
    __shared__ uint32_t t[64][65];
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64, lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int r = ly; r < 64; r += 4) {
        const int64_t i = i0 + r;
        const int c = c0 + lx;
        if (i < n && c < K) t[r][lx] = rank_key(as_prob(scores[i * ld + c], from_logits));
    }
    __syncthreads();
    for (int r = ly; r < 64; r += 4) {
        const int64_t i = i0 + lx;
        const int c = c0 + r;
        if (i < n && c < K) keys[(int64_t)c * n + i] = t[lx][r];
    }
}

// ---- one digit pass: histogram, scan, stable scatter -----------------------------------------------------------------------------------------
// hist[(c, tile, digit)] = rows of the tile whose key holds `digit` at `shift`
__global__ __launch_bounds__(RANK_THREADS) void rank_hist_kernel(const uint32_t *__restrict__ keys, int64_t n, int shift, uint32_t tiles,
                                                                 uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t *k = keys + (int64_t)blockIdx.y * n;
    const int64_t base = (int64_t)blockIdx.x * RANK_TILE;
#pragma unroll
    for (int j = 0; j < RANK_TILE / RANK_THREADS; ++j) {
        const int64_t p = base + j * RANK_THREADS + threadIdx.x;
        if (p < n) atomicAdd(&h[(k[p] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((int64_t)blockIdx.y * tiles + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

// one workgroup per class, thread d = digit d: hist[(c, tile, d)] becomes the rows of digit d in the tiles before `tile`; base[(c, d)] the rows
// of the class whose digit is below d.  ECGVIT_RANK_SCAN_BATCH loads are in flight per step.
__global__ __launch_bounds__(256) void rank_scan_kernel(uint32_t *__restrict__ hist, uint32_t tiles, uint32_t *__restrict__ base) {
    __shared__ uint32_t tot[256];
    const int d = threadIdx.x;
    uint32_t *h = hist + (int64_t)blockIdx.x * tiles * 256 + d;
    uint32_t run = 0;
    for (uint32_t t0 = 0; t0 < tiles; t0 += ECGVIT_RANK_SCAN_BATCH) {
        uint32_t v[ECGVIT_RANK_SCAN_BATCH];
#pragma unroll
        for (int j = 0; j < ECGVIT_RANK_SCAN_BATCH; ++j) v[j] = t0 + j < tiles ? h[(int64_t)(t0 + j) * 256] : 0u;
#pragma unroll
        for (int j = 0; j < ECGVIT_RANK_SCAN_BATCH; ++j) {
            if (t0 + j < tiles) h[(int64_t)(t0 + j) * 256] = run;
            run += v[j];
        }
    }
    tot[d] = run;
    __syncthreads();
    uint32_t b = 0;
    for (int j = 0; j < d; ++j) b += tot[j];
    base[blockIdx.x * 256 + d] = b;
}

// the lanes of the wave that hold a valid row with this lane's digit
__device__ __forceinline__ uint64_t rank_match(uint32_t d, bool valid) {
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// stable: wave w owns rows [w, w + 1) * RANK_WAVE_ROWS of the tile in 64-row steps; a row goes to
//   base[digit] + (rows of the digit in earlier tiles) + (in earlier waves of this tile) + (in earlier steps of this wave) + (in lower lanes of this step).
// idx_in null: the record index is the position (first pass).
__global__ __launch_bounds__(RANK_THREADS) void rank_scatter_kernel(const uint32_t *__restrict__ keys_in, const uint32_t *__restrict__ idx_in, int64_t n,
                                                                    int shift, uint32_t tiles, const uint32_t *__restrict__ hist,
                                                                    const uint32_t *__restrict__ base, uint32_t *__restrict__ keys_out,
                                                                    uint32_t *__restrict__ idx_out) {
    __shared__ uint32_t cnt[4][256];
    const int c = blockIdx.y, w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int64_t row0 = (int64_t)c * n, p0 = (int64_t)blockIdx.x * RANK_TILE + w * RANK_WAVE_ROWS + l;
    const uint64_t below = (1ull << l) - 1ull;
#pragma unroll
    for (int i = 0; i < 4; ++i) cnt[i][threadIdx.x] = 0;
    __syncthreads();
    uint32_t key[RANK_STEPS], rank[RANK_STEPS];   // rank: lower lanes of the step with the digit | rows of the step with the digit << 8 | first lane of them << 16
#pragma unroll
    for (int j = 0; j < RANK_STEPS; ++j) {
        const int64_t p = p0 + j * WAVE;
        const bool valid = p < n;
        key[j] = valid ? keys_in[row0 + p] : 0u;
        const uint32_t d = (key[j] >> shift) & 255u;
        const uint64_t m = rank_match(d, valid);
        const bool first = valid && (m & below) == 0;
        rank[j] = (uint32_t)__popcll(m & below) | ((uint32_t)__popcll(m) << 8) | ((uint32_t)first << 16);
        if (first) cnt[w][d] += rank[j] >> 8 & 0xFFu;   // one lane per digit and wave: no two lanes meet on a counter
        __syncthreads();
    }
    {
        const int d = threadIdx.x;
        uint32_t b = base[c * 256 + d] + hist[((int64_t)c * tiles + blockIdx.x) * 256 + d];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = cnt[i][d];
            cnt[i][d] = b;
            b += x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RANK_STEPS; ++j) {
        const int64_t p = p0 + j * WAVE;
        const bool valid = p < n;
        const uint32_t d = (key[j] >> shift) & 255u;
        const uint32_t at = valid ? cnt[w][d] + (rank[j] & 0xFFu) : 0u;
        const uint32_t idx = !valid ? 0u : idx_in ? idx_in[row0 + p] : (uint32_t)p;
        __syncthreads();
        if (valid && at < n) {
            keys_out[row0 + at] = key[j];
            idx_out[row0 + at] = idx;
        }
        if (rank[j] >> 16) cnt[w][d] += rank[j] >> 8 & 0xFFu;
        __syncthreads();
    }
}

// sorted (key, record index) -> the packed word of every position, and the first position of NaN's key
__global__ __launch_bounds__(RANK_THREADS) void rank_pack_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                                                                 const float *__restrict__ labels, int64_t ldl, int64_t n, uint32_t *__restrict__ packed,
                                                                 int32_t *__restrict__ first_nan) {
    const int c = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * RANK_THREADS + threadIdx.x;
    if (p >= n) return;
    const uint32_t *k = keys + (int64_t)c * n;
    const uint32_t key = k[p], i = idx[(int64_t)c * n + p] & RANK_INDEX_MASK;
    const bool last = p == n - 1 || k[p + 1] != key;
    uint32_t word = i;
    if (i < n && labels[(int64_t)i * ldl + c] != 0.f) word |= RANK_LABEL_BIT;
    if (last) word |= RANK_LAST_BIT;
    packed[(int64_t)c * n + p] = word;
    // exactly one writer per class: NaN's key is the largest, so its positions are the tail of the order
    if (key == RANK_NAN_KEY && (p == 0 || k[p - 1] != RANK_NAN_KEY)) first_nan[c] = (int32_t)p;
    if (p == n - 1 && key != RANK_NAN_KEY) first_nan[c] = (int32_t)n;
}

// ---- replicates: multiplicities --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rank_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    return z;
}
#define RANK_GAMMA 0x9E3779B97F4A7C15ull

// indices non-null: draws given; else draw j of replicate first + r from the generator of the header.  mult is record-major, (n, R4): the
// replicates of one record lie beside each other, where the walk gathers them with one 16-byte load
__global__ __launch_bounds__(256) void rank_multiplicity_kernel(const int64_t *__restrict__ indices, int64_t ld, uint64_t seed, int64_t first, int64_t R,
                                                                int64_t n, uint32_t *__restrict__ mult) {
    const int64_t total = R * n, R4 = rank_pad4(R);
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / n, j = e - r * n;
        uint64_t i;
        if (indices) {
            i = (uint64_t)indices[r * ld + j];
        } else {
            const uint64_t u = rank_mix(rank_mix(seed + RANK_GAMMA * (uint64_t)(first + r + 1)) + RANK_GAMMA * (uint64_t)(j + 1));
            i = __umul64hi(u, (uint64_t)n);
        }
        if (i < (uint64_t)n) atomicAdd(mult + (int64_t)i * R4 + r, 1u);
    }
}

// ---- the weighted rank sum ---------------------------------------------------------------------------------------------------------------------
// The walk skeleton is metrics_common.h's.  State per replicate, wave-uniform: the running sums of the positives' and the negatives' weights
// (P, A = Cn) and their values at the last closed tie group (Pc, Ac): the open group's weights are P - Pc and A - Ac.  A position that closes a
// group adds (P - P') * (A' + A), with P', A' the sums at the closing position before it: sum over the group's positives of
// w * (Cn before the group + Cn at its end).
// A step is ECGVIT_RANK_WALK_ROWS positions, V = 4 consecutive ones per lane: a lane sums its own (first pass, relative to its first position,
// remembering the sums at its last closing position), one exclusive wave scan per sum places the lane, the sums at the last closing position
// before the lane come from the highest lower lane that holds one (a shuffle) or from the carry, and a second pass over the lane's positions adds
// the products.  The V loads of a step are in flight together, and the four waves of a workgroup read neighbouring quarters of the same lines.
// The placement is written out here and in prc_walk_kernel: as a shared function, in each of three forms, it cost a walk 1 to 10 % of its time
// (profiles/r33_walk_skeleton.txt).
__global__ __launch_bounds__(WALK_THREADS) void rank_walk_kernel(const uint32_t *__restrict__ packed, const int32_t *__restrict__ first_nan, int64_t n, int K,
                                                                 const uint32_t *__restrict__ mult, int64_t R, long long *__restrict__ out,
                                                                 long long *__restrict__ pairs) {
    constexpr int G = ECGVIT_RANK_GROUP, V = ECGVIT_RANK_WALK_ROWS / WAVE;
    const WalkWave wv(packed, n, R);
    if (wv.r0 >= R) return;   // wave-uniform; the kernel holds no barrier
    const int l = wv.l;
    const int64_t nan0 = first_nan[wv.c];
    uint32_t P[G], A[G], Pc[G], Ac[G], tp[G], tn[G];
    uint64_t acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) P[g] = A[g] = Pc[g] = Ac[g] = tp[g] = tn[g] = 0u, acc[g] = 0ull;
    for (int64_t b = 0; b < n; b += ECGVIT_RANK_WALK_ROWS) {
        const int64_t p0 = b + (int64_t)l * V;
        uint32_t word[V], w[V][G];
#pragma unroll
        for (int j = 0; j < V; ++j) word[j] = p0 + j < n ? wv.order[p0 + j] : 0u;   // past the end: no label, no closing, weight 0
#pragma unroll
        for (int j = 0; j < V; ++j) walk_weights(wv, word[j], p0 + j < n, n, mult, R, w[j]);
        bool any = false;
#pragma unroll
        for (int j = 0; j < V; ++j) any |= (word[j] & RANK_LAST_BIT) != 0;
        const WalkCloses k = walk_closes(any, wv.below);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            uint32_t sp = 0, sa = 0, cp = 0, ca = 0;   // the lane's sums, and their values at its last closing position
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool pos = word[j] & RANK_LABEL_BIT;
                tp[g] += pos ? w[j][g] : 0u;
                tn[g] += pos ? 0u : w[j][g];
                if (p0 + j >= nan0) w[j][g] = 0u;   // NaN's key: counted in wp / wn above, never in a sum below
                sp += pos ? w[j][g] : 0u;
                sa += pos ? 0u : w[j][g];
                if (word[j] & RANK_LAST_BIT) cp = sp, ca = sa;
            }
            const uint32_t p_in = P[g] + walk_scan(sp, l) - sp, a_in = A[g] + walk_scan(sa, l) - sa;   // the sums before the lane
            const uint32_t p_cl = p_in + cp, a_cl = a_in + ca;
            const uint32_t p_sh = __shfl(p_cl, k.prev, WAVE), a_sh = __shfl(a_cl, k.prev, WAVE);
            uint32_t pc = k.before ? p_sh : Pc[g], ac = k.before ? a_sh : Ac[g], pr = p_in, ar = a_in;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const bool pos = word[j] & RANK_LABEL_BIT;
                pr += pos ? w[j][g] : 0u;
                ar += pos ? 0u : w[j][g];
                if (word[j] & RANK_LAST_BIT) {
                    acc[g] += (uint64_t)(pr - pc) * ((uint64_t)ac + ar);
                    pc = pr, ac = ar;
                }
            }
            const uint32_t p_top = __shfl(p_cl, k.top, WAVE), a_top = __shfl(a_cl, k.top, WAVE);
            if (k.closes) Pc[g] = p_top, Ac[g] = a_top;
            P[g] = __shfl(p_in + sp, 63, WAVE), A[g] = __shfl(a_in + sa, 63, WAVE);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint64_t num2 = walk_sum(acc[g]), wp = walk_sum<uint64_t>(tp[g]), wn = walk_sum<uint64_t>(tn[g]);
        if (l == 0 && wv.r0 + g < R) {
            long long *o = out + ((wv.r0 + g) * K + wv.c) * 3;
            o[0] = (long long)num2, o[1] = (long long)wp, o[2] = (long long)wn;
            if (pairs) pairs[wv.c] = (long long)num2;
        }
    }
}

// ---- entry points --------------------------------------------------------------------------------------------------------------------------------
static inline int64_t rank_align(int64_t b) { return (b + 255) & ~(int64_t)255; }
static inline int64_t rank_tiles(int64_t n) { return (n + RANK_TILE - 1) / RANK_TILE; }

extern "C" int64_t ecgvit_rank_workspace(int64_t n, int K, int64_t R) {
    if (!rank_shape_ok(n, K) || R < 0 || R > ECGVIT_RANK_MAX_REPLICATES) return 0;
    if (R > 0) return rank_align(rank_pad4(R) * n * 4);
    return 4 * rank_align((int64_t)K * n * 4) + rank_align((int64_t)K * rank_tiles(n) * 256 * 4) + rank_align((int64_t)K * 256 * 4);
}

extern "C" int ecgvit_rank_sort(const float *scores, int64_t ld, const float *labels, int64_t ldl, int64_t n, int K, int from_logits, uint32_t *packed,
                                int32_t *first_nan, void *workspace, void *stream) {
    if (!rank_shape_ok(n, K) || ld < K || ldl < K || !scores || !labels || !packed || !first_nan || !workspace) return ECGVIT_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return ECGVIT_EINVAL;
    hipStream_t s = as_stream(stream);
    const int64_t plane = rank_align((int64_t)K * n * 4);
    const uint32_t tiles = (uint32_t)rank_tiles(n);
    char *ws = static_cast<char *>(workspace);
    uint32_t *key[2] = {reinterpret_cast<uint32_t *>(ws), reinterpret_cast<uint32_t *>(ws + plane)};
    uint32_t *idx[2] = {reinterpret_cast<uint32_t *>(ws + 2 * plane), reinterpret_cast<uint32_t *>(ws + 3 * plane)};
    uint32_t *hist = reinterpret_cast<uint32_t *>(ws + 4 * plane);
    uint32_t *base = reinterpret_cast<uint32_t *>(ws + 4 * plane + rank_align((int64_t)K * tiles * 256 * 4));
    rank_keys_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)((K + 63) / 64)), RANK_THREADS, 0, s>>>(scores, ld, n, K, from_logits, key[0]);
    ECGVIT_CHECK_LAUNCH();
    for (int pass = 0; pass < 4; ++pass) {   // an even number of passes: the sorted planes are key[0], idx[0]
        const int in = pass & 1, shift = 8 * pass;
        rank_hist_kernel<<<dim3(tiles, K), RANK_THREADS, 0, s>>>(key[in], n, shift, tiles, hist);
        ECGVIT_CHECK_LAUNCH();
        rank_scan_kernel<<<K, 256, 0, s>>>(hist, tiles, base);
        ECGVIT_CHECK_LAUNCH();
        rank_scatter_kernel<<<dim3(tiles, K), RANK_THREADS, 0, s>>>(key[in], pass ? idx[in] : nullptr, n, shift, tiles, hist, base, key[in ^ 1], idx[in ^ 1]);
        ECGVIT_CHECK_LAUNCH();
    }
    rank_pack_kernel<<<dim3((unsigned)((n + RANK_THREADS - 1) / RANK_THREADS), K), RANK_THREADS, 0, s>>>(key[0], idx[0], labels, ldl, n, packed, first_nan);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

static int rank_multiplicities(const int64_t *indices, int64_t ld, uint64_t seed, int64_t first, int64_t R, int64_t n, uint32_t *mult, void *stream) {
    if (n < 1 || n > ECGVIT_RANK_MAX_ROWS || R < 1 || R > ECGVIT_RANK_MAX_REPLICATES || first < 0 || !mult || (reinterpret_cast<uintptr_t>(mult) & 15)) return ECGVIT_EINVAL;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(mult, 0, sizeof(uint32_t) * (size_t)rank_pad4(R) * (size_t)n, s) != hipSuccess) return ECGVIT_ELAUNCH;
    const int64_t blocks = (R * n + 255) / 256;
    rank_multiplicity_kernel<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), 256, 0, s>>>(indices, ld, seed, first, R, n, mult);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

extern "C" int ecgvit_rank_multiplicities(const int64_t *indices, int64_t ld, int64_t R, int64_t n, uint32_t *mult, void *stream) {
    if (!indices || ld < n) return ECGVIT_EINVAL;
    return rank_multiplicities(indices, ld, 0, 0, R, n, mult, stream);
}

extern "C" int ecgvit_rank_multiplicities_seeded(uint64_t seed, int64_t first, int64_t R, int64_t n, uint32_t *mult, void *stream) {
    return rank_multiplicities(nullptr, 0, seed, first, R, n, mult, stream);
}

extern "C" int ecgvit_rank_walk(const uint32_t *packed, const int32_t *first_nan, int64_t n, int K, const uint32_t *mult, int64_t R, int64_t *out,
                                int64_t *pairs, void *stream) {
    if (!walk_args_ok(packed, first_nan, n, K, mult, R, out) || (pairs && R != 1)) return ECGVIT_EINVAL;
    rank_walk_kernel<<<walk_grid(R, K), WALK_THREADS, 0, as_stream(stream)>>>(packed, first_nan, n, K, mult, R, reinterpret_cast<long long *>(out),
                                                                              reinterpret_cast<long long *>(pairs));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
