// Per-lead statistics of a record store, for fitting the input normalisation on the device (transform.fit_dynamic_normalize; the reference's
// DynamicNormalize, preprocess/transform.py:38-137): counts, f64 moments and EXACT order statistics by radix select.  HBM-bound passes: every
// selected sample is read once per pass, nothing is written but a few hundred counters.
//
// Addressing is that of ecgvit_patch_gather_transform_varlen: lead c of record r = raw_len[r] f32 samples at x + src_off[r] + c * lead_stride.
// A record's first sample sits at any 4-byte address: each (record, lead) run is read as a scalar head up to the next 16-byte boundary, 16-byte
// loads, and a scalar tail.  Workgroup (g, c) of a FIT_GROUPS x C grid reads lead c of records g, g + G, g + 2 G, ...: one lead per workgroup,
// so whatever it compares a sample against (the mean, the targets' key prefixes) is uniform.
#include "common.h"

#define FIT_THREADS 256
#define FIT_GROUPS 512     // record groups per lead (fewer when there are fewer records)
#define FIT_TARGETS ECGVIT_FIT_TARGETS   // order statistics per lead and select
#define FIT_BINS ECGVIT_FIT_BINS         // 8-bit digits: four passes over the 32-bit key
#define FIT_REPS 32        // copies of every bin in the top-digit pass (see fit_hist_top_kernel)

typedef unsigned long long u64;

// fn(sample) for every sample of the run p[0 .. n), each once, by the FIT_THREADS threads of the workgroup
template <typename F> __device__ __forceinline__ void fit_for_each(const float *__restrict__ p, int n, F fn) {
    const int tid = threadIdx.x;
    int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    if (tid < head) fn(p[tid]);
    const f32x4 *__restrict__ q = reinterpret_cast<const f32x4 *>(p + head);
    const int nv = (n - head) >> 2;
    int i = tid;
    for (; i + FIT_THREADS < nv; i += 2 * FIT_THREADS) {   // two independent 16-B loads in flight
        const f32x4 a = q[i], b = q[i + FIT_THREADS];
        fn(a[0]); fn(a[1]); fn(a[2]); fn(a[3]);
        fn(b[0]); fn(b[1]); fn(b[2]); fn(b[3]);
    }
    if (i < nv) {
        const f32x4 a = q[i];
        fn(a[0]); fn(a[1]); fn(a[2]); fn(a[3]);
    }
    const int t0 = head + 4 * nv;
    if (t0 + tid < n) fn(p[t0 + tid]);
}

// the monotone key: a < b as floats <=> key(a) < key(b), with -0.0 directly below +0.0; denormals and +-inf are ordinary keys
__device__ __forceinline__ uint32_t fit_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}

// =====================================================================================================
// moments.  Stage one: per workgroup the count of non-NaN samples, the count of NaN samples and the f64 sum of (x - shift) or of (x - shift)^2
// over its records, each thread adding in the order it reads, the threads meeting in a fixed tree.  Stage two: one workgroup per lead adds the
// G partials in a fixed order and adds the result to the caller's state.  No floating-point atomics: the same launches give the same bits.
// =====================================================================================================
struct FitPartial { u64 n, nan; double s; double pad; };

__device__ __forceinline__ double fit_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 fit_wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <bool SQ>
__global__ __launch_bounds__(FIT_THREADS) void fit_moments_kernel(const float *__restrict__ x, const int64_t *__restrict__ src_off, int64_t lead_stride,
                                                                   const int32_t *__restrict__ raw_len, int R, const double *__restrict__ mean,
                                                                   FitPartial *__restrict__ part) {
    __shared__ double sd[FIT_THREADS / WAVE];
    __shared__ u64 sn[FIT_THREADS / WAVE], sq[FIT_THREADS / WAVE];
    const int c = blockIdx.y, G = gridDim.x;
    const double mu = SQ ? mean[c] : 0.0;
    double s = 0.0;
    u64 n = 0, nan = 0;
    for (int r = blockIdx.x; r < R; r += G) {
        const int len = raw_len[r];
        if (len <= 0) continue;
        fit_for_each(x + src_off[r] + (int64_t)c * lead_stride, len, [&](float v) {
            if (v != v) {
                ++nan;
            } else {
                ++n;
                if (SQ) {
                    const double d = (double)v - mu;
                    s += d * d;
                } else {
                    s += (double)v;
                }
            }
        });
    }
    s = fit_wave_sum(s);
    n = fit_wave_sum(n);
    nan = fit_wave_sum(nan);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sd[w] = s; sn[w] = n; sq[w] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        FitPartial o;
        o.s = ((sd[0] + sd[1]) + sd[2]) + sd[3];
        o.n = sn[0] + sn[1] + sn[2] + sn[3];
        o.nan = sq[0] + sq[1] + sq[2] + sq[3];
        o.pad = 0.0;
        part[(int64_t)c * G + blockIdx.x] = o;
    }
}

// state per lead: { u64 count, u64 nan_count, f64 sum, f64 sum of squared deviations }.  SQ adds to the last alone (the counts were taken with the sum)
template <bool SQ>
__global__ __launch_bounds__(FIT_THREADS) void fit_moments_finish_kernel(const FitPartial *__restrict__ part, int G, u64 *__restrict__ state) {
    __shared__ double sd[FIT_THREADS / WAVE];
    __shared__ u64 sn[FIT_THREADS / WAVE], sq[FIT_THREADS / WAVE];
    const int c = blockIdx.x;
    double s = 0.0;
    u64 n = 0, nan = 0;
    for (int g = threadIdx.x; g < G; g += FIT_THREADS) {
        const FitPartial p = part[(int64_t)c * G + g];
        s += p.s; n += p.n; nan += p.nan;
    }
    s = fit_wave_sum(s);
    n = fit_wave_sum(n);
    nan = fit_wave_sum(nan);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sd[w] = s; sn[w] = n; sq[w] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = ((sd[0] + sd[1]) + sd[2]) + sd[3];
        double *fs = reinterpret_cast<double *>(state + 4 * c);
        if (SQ) {
            fs[3] += t;
        } else {
            state[4 * c] += sn[0] + sn[1] + sn[2] + sn[3];
            state[4 * c + 1] += sq[0] + sq[1] + sq[2] + sq[3];
            fs[2] += t;
        }
    }
}

// =====================================================================================================
// radix select, pass 0: the histogram of the key's top 8 bits over every non-NaN sample of the lead.  The top digit is the sign and seven
// exponent bits: ECG samples fall into a handful of bins whatever their distribution, and a zero-padded store into ONE.  So every bin has
// FIT_REPS = 32 copies, a lane adds to copy (lane & 31), and copy r of bin b sits at word b * 32 + ((r + b) & 31): the 64 lanes of a wave hit
// a given address at most twice, and the copies of one bin lie in 32 different banks -- the integer LDS atomics do not serialise on a hot bin
// and no lane votes or compares.  32 KiB of LDS per workgroup.  u32 counters: flushed (u64 vector atomics, non-zero bins only) before the
// samples counted since the last flush could pass 2^32, and at the end.
// =====================================================================================================
__device__ __forceinline__ void fit_flush_top(uint32_t *lh, u64 *__restrict__ gh) {
    __syncthreads();
    const int b = threadIdx.x;   // FIT_THREADS == FIT_BINS
    u64 t = 0;
#pragma unroll 8
    for (int r = 0; r < FIT_REPS; ++r) {
        const int a = b * FIT_REPS + ((r + b) & (FIT_REPS - 1));
        t += lh[a];
        lh[a] = 0;
    }
    if (t) atomicAdd(gh + b, t);
    __syncthreads();
}

__global__ __launch_bounds__(FIT_THREADS) void fit_hist_top_kernel(const float *__restrict__ x, const int64_t *__restrict__ src_off, int64_t lead_stride,
                                                                    const int32_t *__restrict__ raw_len, int R, u64 *__restrict__ hist) {
    __shared__ uint32_t lh[FIT_BINS * FIT_REPS];
    for (int i = threadIdx.x; i < FIT_BINS * FIT_REPS; i += FIT_THREADS) lh[i] = 0;
    __syncthreads();
    const int c = blockIdx.y, G = gridDim.x;
    u64 *gh = hist + (int64_t)c * FIT_TARGETS * FIT_BINS;   // slot 0 of the lead
    const uint32_t rep = threadIdx.x & (FIT_REPS - 1);
    u64 since = 0;
    for (int r = blockIdx.x; r < R; r += G) {
        const int len = raw_len[r];
        if (len <= 0) continue;
        if (since + (u64)len > 0xFFFFFFFFull) {
            fit_flush_top(lh, gh);
            since = 0;
        }
        since += (u64)len;
        fit_for_each(x + src_off[r] + (int64_t)c * lead_stride, len, [&](float v) {
            if (v == v) {
                const uint32_t b = fit_key(v) >> 24;
                atomicAdd(&lh[b * FIT_REPS + ((rep + b) & (FIT_REPS - 1))], 1u);
            }
        });
    }
    fit_flush_top(lh, gh);
}

// =====================================================================================================
// passes 1..3: the histogram of the next 8 bits over the samples whose key starts with a target's prefix.  sel (per lead, per target, 4 x u64):
// { remaining rank, key prefix (the decided bits, in place), slot, count of the chosen bin }; targets with one prefix share the slot of the
// first of them, and a sample is counted once, in that slot.  Most samples match nothing; those that do spread over the 256 bins of their
// slot, except equal samples (ties, the zeros of a padded store), which all want one counter: up to FIT_PEEL times the lanes that share the
// first matching lane's counter are added as ONE atomic of their number, the rest add one by one.
// =====================================================================================================
#define FIT_PEEL 3

__device__ __forceinline__ void fit_flush_slots(uint32_t *lh, u64 *__restrict__ gh, int T) {
    __syncthreads();
    for (int i = threadIdx.x; i < T * FIT_BINS; i += FIT_THREADS) {
        const uint32_t t = lh[i];
        lh[i] = 0;
        if (t) atomicAdd(gh + i, (u64)t);
    }
    __syncthreads();
}

__global__ __launch_bounds__(FIT_THREADS) void fit_hist_next_kernel(const float *__restrict__ x, const int64_t *__restrict__ src_off, int64_t lead_stride,
                                                                     const int32_t *__restrict__ raw_len, int R, const u64 *__restrict__ sel, int T,
                                                                     int pass, u64 *__restrict__ hist) {
    __shared__ uint32_t lh[FIT_TARGETS * FIT_BINS];
    __shared__ uint32_t want[FIT_TARGETS];
    for (int i = threadIdx.x; i < FIT_TARGETS * FIT_BINS; i += FIT_THREADS) lh[i] = 0;
    const int c = blockIdx.y, G = gridDim.x;
    const int sh = 32 - 8 * pass;   // the decided bits are key >> sh: at most 24 of them, so 0xFFFFFFFF matches no sample
    if (threadIdx.x < FIT_TARGETS) {
        const u64 *s = sel + ((int64_t)c * FIT_TARGETS + threadIdx.x) * 4;
        want[threadIdx.x] = (threadIdx.x < T && s[2] == (u64)threadIdx.x) ? (uint32_t)s[1] >> sh : 0xFFFFFFFFu;
    }
    __syncthreads();
    uint32_t w[FIT_TARGETS];
#pragma unroll
    for (int t = 0; t < FIT_TARGETS; ++t) w[t] = want[t];
    u64 *gh = hist + (int64_t)c * FIT_TARGETS * FIT_BINS;
    const int lane = threadIdx.x & 63;
    u64 since = 0;
    for (int r = blockIdx.x; r < R; r += G) {
        const int len = raw_len[r];
        if (len <= 0) continue;
        if (since + (u64)len > 0xFFFFFFFFull) {
            fit_flush_slots(lh, gh, T);
            since = 0;
        }
        since += (u64)len;
        fit_for_each(x + src_off[r] + (int64_t)c * lead_stride, len, [&](float v) {
            const uint32_t key = fit_key(v), pre = key >> sh;
            int slot = -1;
#pragma unroll
            for (int t = 0; t < FIT_TARGETS; ++t) slot = (pre == w[t]) ? t : slot;   // at most one slot holds a given prefix
            bool todo = slot >= 0 && v == v;
            const uint32_t idx = (uint32_t)slot * FIT_BINS + ((key >> (sh - 8)) & 0xFFu);
#pragma unroll
            for (int it = 0; it < FIT_PEEL; ++it) {
                if (todo) {
                    const uint32_t first = __builtin_amdgcn_readfirstlane(idx);
                    const bool same = idx == first;
                    const u64 m = __ballot(same);
                    if (same) {
                        if (lane == __ffsll((long long)m) - 1) atomicAdd(&lh[first], (uint32_t)__popcll(m));
                        todo = false;
                    }
                }
            }
            if (todo) atomicAdd(&lh[idx], 1u);
        });
    }
    fit_flush_slots(lh, gh, T);
}

// =====================================================================================================
// the scan between two passes, on the device: thread t of lead c walks the 256 bins of target t's slot, finds the bin that holds its remaining
// rank, and writes the bin into the prefix, the rank within the bin and the bin's count back; then the targets are regrouped by their new
// prefix.  After pass 3 the prefix is the whole key of the exact order statistic.
// =====================================================================================================
__global__ __launch_bounds__(WAVE) void fit_select_kernel(const u64 *__restrict__ hist, u64 *__restrict__ sel, int T, int pass) {
    __shared__ uint32_t pre[FIT_TARGETS];
    const int c = blockIdx.x, t = threadIdx.x;
    u64 *s = sel + ((int64_t)c * FIT_TARGETS + t) * 4;
    if (t < T) {
        const u64 rank = s[0];
        const u64 *h = hist + ((int64_t)c * FIT_TARGETS + (pass == 0 ? 0 : (int)s[2])) * FIT_BINS;
        u64 cum = 0, rem = 0, cnt = 0;
        int bin = FIT_BINS - 1;
        bool found = false;
#pragma unroll 8
        for (int b = 0; b < FIT_BINS; ++b) {
            const u64 n = h[b];
            if (!found && rank < cum + n) {
                found = true;
                bin = b; rem = rank - cum; cnt = n;
            }
            cum += n;
        }
        const uint32_t p = (pass == 0 ? 0u : (uint32_t)s[1]) | ((uint32_t)bin << (24 - 8 * pass));
        s[0] = rem;
        s[1] = p;
        s[3] = found ? cnt : 0;   // 0: the rank was not below the count of the samples (a caller's error; the host checks it)
        pre[t] = p;
    }
    __syncthreads();
    if (t < T) {
        int slot = t;
        for (int j = t - 1; j >= 0; --j) slot = pre[j] == pre[t] ? j : slot;
        s[2] = (u64)slot;
    }
}

// =====================================================================================================
// entry points
// =====================================================================================================
static inline int fit_groups(int R) { return R < FIT_GROUPS ? R : FIT_GROUPS; }

int64_t ecgvit_fit_workspace(int R, int C) {
    if (R <= 0 || C <= 0) return 0;
    return (int64_t)C * fit_groups(R) * (int64_t)sizeof(FitPartial);
}

static bool fit_args_ok(const float *x, const int64_t *src_off, const int32_t *raw_len, int R, int C) {
    return x && src_off && raw_len && R > 0 && C > 0 && C <= 65535 && (reinterpret_cast<uintptr_t>(x) & 3u) == 0;
}

int ecgvit_fit_moments(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, const double *mean,
                       void *workspace, void *state, void *stream) {
    if (!fit_args_ok(x, src_off, raw_len, R, C) || !workspace || !state) return ECGVIT_EINVAL;
    const int G = fit_groups(R);
    FitPartial *part = reinterpret_cast<FitPartial *>(workspace);
    if (mean) {
        hipLaunchKernelGGL(fit_moments_kernel<true>, dim3(G, C), dim3(FIT_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, R, mean, part);
        ECGVIT_CHECK_LAUNCH();
        hipLaunchKernelGGL(fit_moments_finish_kernel<true>, dim3(C), dim3(FIT_THREADS), 0, as_stream(stream), part, G, reinterpret_cast<u64 *>(state));
    } else {
        hipLaunchKernelGGL(fit_moments_kernel<false>, dim3(G, C), dim3(FIT_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, R, mean, part);
        ECGVIT_CHECK_LAUNCH();
        hipLaunchKernelGGL(fit_moments_finish_kernel<false>, dim3(C), dim3(FIT_THREADS), 0, as_stream(stream), part, G, reinterpret_cast<u64 *>(state));
    }
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_fit_histogram(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, const uint64_t *sel,
                         int ntarget, int pass, uint64_t *hist, void *stream) {
    if (!fit_args_ok(x, src_off, raw_len, R, C) || !hist || pass < 0 || pass > 3) return ECGVIT_EINVAL;
    if (pass > 0 && (!sel || ntarget < 1 || ntarget > FIT_TARGETS)) return ECGVIT_EINVAL;
    const int G = fit_groups(R);
    if (pass == 0)
        hipLaunchKernelGGL(fit_hist_top_kernel, dim3(G, C), dim3(FIT_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, R,
                           reinterpret_cast<u64 *>(hist));
    else
        hipLaunchKernelGGL(fit_hist_next_kernel, dim3(G, C), dim3(FIT_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, R,
                           reinterpret_cast<const u64 *>(sel), ntarget, pass, reinterpret_cast<u64 *>(hist));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_fit_select(const uint64_t *hist, uint64_t *sel, int C, int ntarget, int pass, void *stream) {
    if (!hist || !sel || C <= 0 || ntarget < 1 || ntarget > FIT_TARGETS || pass < 0 || pass > 3) return ECGVIT_EINVAL;
    hipLaunchKernelGGL(fit_select_kernel, dim3(C), dim3(WAVE), 0, as_stream(stream), reinterpret_cast<const u64 *>(hist), reinterpret_cast<u64 *>(sel),
                       ntarget, pass);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
