// The Zheng et al. denoiser (denoise.py; the reference's preprocess/data_preprocessor.py): zero-phase low-pass, the noise estimate and non-local
// means, per (record, lead), over a record store addressed as fit_stats.hip addresses it.  Contracts and the order of every sum: include/ecgvit_hip.h.
//
// One workgroup per (record, lead) in all three kernels.  The low-pass and the noise estimate are sequential recurrences in f64: lane 0 walks
// them chunk by chunk through LDS while the whole workgroup moves the chunks (coalesced), and their f64 intermediates live in a caller's
// workspace.  Non-local means is the hot path: the lead sits in LDS as f32, a lane owns runs of NLM_RUN consecutive output samples.
#include "common.h"

#define DN_MAX_LEN 32768            // samples per record: 128 KiB of f32 in LDS for the non-local means
#define DN_WS_PAD 64                // workspace doubles per lead beyond max_len (the low-pass's two extensions: 2 * 3 * 9 = 54)
#define DN_MAX_TAPS 9

static bool dn_store_ok(const float *x, const int64_t *src_off, const int32_t *raw_len, int R, int C, int max_len) {
    return x && src_off && raw_len && R > 0 && C > 0 && C <= 65535 && max_len > 0 && max_len <= DN_MAX_LEN && (reinterpret_cast<uintptr_t>(x) & 3u) == 0 &&
           (reinterpret_cast<uintptr_t>(src_off) & 7u) == 0 && (reinterpret_cast<uintptr_t>(raw_len) & 3u) == 0;
}

int64_t ecgvit_denoise_workspace(int R, int C, int max_len) {
    if (R <= 0 || C <= 0 || max_len <= 0 || max_len > DN_MAX_LEN) return 0;
    return (int64_t)R * C * (max_len + DN_WS_PAD) * 8;
}

// =====================================================================================================
// zero-phase IIR filter (scipy.signal.filtfilt with its defaults)
// =====================================================================================================
#define FF_THREADS 64
#define FF_CHUNK 512

struct FiltArgs {
    const float *x;
    float *out;
    const int64_t *src_off;
    int64_t lead_stride;
    const int32_t *raw_len;
    double *ws;
    int C, max_len, ntaps;
    double b[DN_MAX_TAPS], a[DN_MAX_TAPS], zi[DN_MAX_TAPS - 1];   // taps past ntaps are 0: the state they feed stays 0
};

// one direct-form-II-transposed step, scipy's order: y = z0 + b0 x; z_k = z_{k+1} + x b_{k+1} - y a_{k+1}
__device__ __forceinline__ double ff_step(const FiltArgs &g, double (&z)[DN_MAX_TAPS - 1], double xi) {
    const double y = z[0] + g.b[0] * xi;
#pragma unroll
    for (int k = 0; k < DN_MAX_TAPS - 2; ++k) z[k] = z[k + 1] + xi * g.b[k + 1] - y * g.a[k + 1];
    z[DN_MAX_TAPS - 2] = xi * g.b[DN_MAX_TAPS - 1] - y * g.a[DN_MAX_TAPS - 1];
    return y;
}

__global__ __launch_bounds__(FF_THREADS) void filtfilt_kernel(FiltArgs g) {
    __shared__ double buf[FF_CHUNK];
    const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int n = g.raw_len[r], pad = 3 * g.ntaps;
    if (n <= pad || n > g.max_len) return;       // (the launcher refused min_len <= padlen; a record outside the caller's promise is left alone)
    const int64_t base = g.src_off[r] + (int64_t)c * g.lead_stride;
    const float *x = g.x + base;
    double *ws = g.ws + ((int64_t)r * g.C + c) * (g.max_len + DN_WS_PAD);
    const int m = n + 2 * pad;
    double z[DN_MAX_TAPS - 1];
    // forward over the odd extension: 2 x[0] - x[pad .. 1], x, 2 x[n-1] - x[n-2 .. n-1-pad]
    for (int c0 = 0; c0 < m; c0 += FF_CHUNK) {
        const int cn = min(FF_CHUNK, m - c0);
        for (int i = tid; i < cn; i += FF_THREADS) {
            const int e = c0 + i;
            double v;
            if (e < pad) v = 2.0 * (double)x[0] - (double)x[pad - e];
            else if (e < pad + n) v = (double)x[e - pad];
            else v = 2.0 * (double)x[n - 1] - (double)x[n - 2 - (e - pad - n)];
            buf[i] = v;
        }
        __syncthreads();
        if (tid == 0) {
            if (c0 == 0) {
#pragma unroll
                for (int k = 0; k < DN_MAX_TAPS - 1; ++k) z[k] = g.zi[k] * buf[0];
            }
            for (int i = 0; i < cn; ++i) buf[i] = ff_step(g, z, buf[i]);
        }
        __syncthreads();
        for (int i = tid; i < cn; i += FF_THREADS) ws[c0 + i] = buf[i];
        __syncthreads();
    }
    // backward: the same filter over the reversed run, reversed again and stripped of the extension.  Every sample of x was consumed above, so
    // out may be x.
    float *out = g.out + base;
    for (int c0 = 0; c0 < m; c0 += FF_CHUNK) {
        const int cn = min(FF_CHUNK, m - c0);
        for (int i = tid; i < cn; i += FF_THREADS) buf[i] = ws[m - 1 - (c0 + i)];
        __syncthreads();
        if (tid == 0) {
            if (c0 == 0) {
#pragma unroll
                for (int k = 0; k < DN_MAX_TAPS - 1; ++k) z[k] = g.zi[k] * buf[0];
            }
            for (int i = 0; i < cn; ++i) buf[i] = ff_step(g, z, buf[i]);
        }
        __syncthreads();
        for (int i = tid; i < cn; i += FF_THREADS) {
            const int j = m - 1 - (c0 + i) - pad;
            if (j >= 0 && j < n) out[j] = (float)buf[i];
        }
        __syncthreads();
    }
}

int ecgvit_filtfilt(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                    int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len) || !out || (reinterpret_cast<uintptr_t>(out) & 3u) || !workspace ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) || !b || !a || ntaps < 1 || ntaps > DN_MAX_TAPS || (ntaps > 1 && !zi))
        return ECGVIT_EINVAL;
    if (min_len <= 3 * ntaps || min_len > max_len) return ECGVIT_EINVAL;      // where scipy raises: the run must be longer than padlen
    if (!(a[0] == 1.0)) return ECGVIT_EINVAL;
    FiltArgs g;
    for (int k = 0; k < DN_MAX_TAPS; ++k) {
        g.b[k] = k < ntaps ? b[k] : 0.0;
        g.a[k] = k < ntaps ? a[k] : 0.0;
        if (k < DN_MAX_TAPS - 1) g.zi[k] = k < ntaps - 1 ? zi[k] : 0.0;
        if (!(g.b[k] - g.b[k] == 0.0) || !(g.a[k] - g.a[k] == 0.0) || (k < DN_MAX_TAPS - 1 && !(g.zi[k] - g.zi[k] == 0.0))) return ECGVIT_EINVAL;   // finite
    }
    g.x = x; g.out = out; g.src_off = src_off; g.lead_stride = lead_stride; g.raw_len = raw_len; g.ws = reinterpret_cast<double *>(workspace);
    g.C = C; g.max_len = max_len; g.ntaps = ntaps;
    hipLaunchKernelGGL(filtfilt_kernel, dim3(R, C), dim3(FF_THREADS), 0, as_stream(stream), g);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

// =====================================================================================================
// noise estimate (the reference's est_noise_std)
// =====================================================================================================
#define SG_THREADS 256
#define SG_CHUNK 1024

__device__ __forceinline__ unsigned long long sg_key(double v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
    return bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double sg_value(unsigned long long key) {
    const unsigned long long bits = key ^ ((key >> 63) ? (1ull << 63) : ~0ull);
    return __longlong_as_double((long long)bits);
}

// the k-th smallest (0-based) of f(ws[0 .. n)) by radix select on the monotone key of the f64 bit pattern, 8 bits a pass: exact.
// DEV: f(v) = |1.4826 (v - m)|, else f(v) = v.  Integer atomics on the LDS histogram only.  Every thread returns the value.
template <bool DEV> __device__ double sg_select(const double *ws, int n, unsigned k, double m, unsigned *hist) {
    unsigned long long prefix = 0;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        for (int b = threadIdx.x; b < 256; b += SG_THREADS) hist[b] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += SG_THREADS) {
            double v = ws[i];
            if (DEV) v = fabs(1.4826 * (v - m));
            const unsigned long long key = sg_key(v);
            if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned cum = 0, below = 0;
        int bin = 255;
        bool found = false;
        for (int b = 0; b < 256; ++b) {
            const unsigned h = hist[b];
            if (!found && k < cum + h) { found = true; bin = b; below = cum; }
            cum += h;
        }
        k -= below;
        prefix = (prefix << 8) | (unsigned long long)bin;
        __syncthreads();
    }
    return sg_value(prefix);
}

template <bool DEV> __device__ double sg_median(const double *ws, int n, double m, unsigned *hist) {
    const double lo = sg_select<DEV>(ws, n, (unsigned)((n - 1) / 2), m, hist);
    const double hi = (n & 1) ? lo : sg_select<DEV>(ws, n, (unsigned)(n / 2), m, hist);
    return (n & 1) ? lo : (lo + hi) / 2.0;
}

__global__ __launch_bounds__(SG_THREADS) void nlm_sigma_kernel(const float *__restrict__ xs, const int64_t *__restrict__ src_off, int64_t lead_stride,
                                                               const int32_t *__restrict__ raw_len, int C, int max_len, double *__restrict__ sigma,
                                                               double *__restrict__ wsa) {
    __shared__ float sx[SG_CHUNK + 1];
    __shared__ double sr[SG_CHUNK];
    __shared__ unsigned hist[256];
    const int r = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int n = raw_len[r];
    if (n <= 0 || n > max_len) return;
    const float *__restrict__ x = xs + src_off[r] + (int64_t)c * lead_stride;
    double *ws = wsa + ((int64_t)r * C + c) * (max_len + DN_WS_PAD);
    // res[i] = (2 res[i] - res[i-1] - res[i+1]) / sqrt(6), i = 1 .. n-2, in place: res[i-1] is the updated value, res[i+1] the original
    double prev = 0.0;
    for (int c0 = 0; c0 < n; c0 += SG_CHUNK) {
        const int cn = min(SG_CHUNK, n - c0);
        for (int i = tid; i < cn + 1; i += SG_THREADS) sx[i] = c0 + i < n ? x[c0 + i] : 0.f;
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < cn; ++i) {
                const int gi = c0 + i;
                double v = (double)sx[i];
                if (gi > 0 && gi < n - 1) v = (2.0 * v - prev - (double)sx[i + 1]) / 2.449489742783178;
                prev = v;
                sr[i] = v;
            }
        }
        __syncthreads();
        for (int i = tid; i < cn; i += SG_THREADS) ws[c0 + i] = sr[i];
        __syncthreads();
    }
    __threadfence_block();
    const double m = sg_median<false>(ws, n, 0.0, hist);
    const double s = sg_median<true>(ws, n, m, hist);
    if (tid == 0) sigma[(int64_t)r * C + c] = s;
}

int ecgvit_nlm_sigma(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                     void *workspace, void *stream) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len) || !sigma || (reinterpret_cast<uintptr_t>(sigma) & 7u) || !workspace ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return ECGVIT_EINVAL;
    hipLaunchKernelGGL(nlm_sigma_kernel, dim3(R, C), dim3(SG_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, C, max_len, sigma,
                       reinterpret_cast<double *>(workspace));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

// =====================================================================================================
// non-local means.  With t0 = ii0 + idx (the neighbour of a run's first sample) as the loop variable instead of the shift idx, the neighbour
// window s[t0 - p .. t0 + RUN - 1 + p] is the SAME for every lane of the workgroup (an LDS broadcast), every bounds decision is uniform, and a
// lane compares it with its own window, which stays in registers.  For one lane t0 ascending is idx ascending: the order the contract fixes.
//   fast body (patch_wd == NLM_P, the whole neighbour window inside the record): no masks, the lane's own window from registers;
//   general body (any patch_wd; t0 within RUN + p of either end; the remainder of the fast range): one t0, every pair masked.
// Runs start NLM_RUN = 15 samples apart: an odd stride, so the 32 lanes of an LDS group read 32 different banks from their own windows.
// The last run of a record is moved back to end on the last output sample (it recomputes a few samples of its neighbour and stores only its own),
// so that every lane of a record longer than one run takes the fast body for the same t0.
// =====================================================================================================
#define NLM_RUN 15
#define NLM_P 10
#define NLM_U 1                     // t0 per neighbour-window load of the fast body: 1 keeps the kernel at 158 VGPRs, three waves per SIMD (4: 256)
#define NLM_WN (NLM_RUN + 2 * NLM_P)
#define NLM_MAX_THREADS 512

struct NlmArgs {
    const float *x;
    float *out;
    const int64_t *src_off;
    int64_t lead_stride;
    const int32_t *raw_len;
    const double *sigma;
    double scale;
    int C, p, W, max_len;
};

// one t0 for the run that starts at output sample a and holds len samples; pairs whose neighbour index falls outside [0, n) contribute 0
__device__ __forceinline__ void nlm_general(const float *s, int n, int p, int a, int len, int t0, float cexp, float (&acc)[NLM_RUN], float (&z)[NLM_RUN]) {
    float d = 0.f;
    for (int j = -p; j <= p; ++j) {
        const int k = t0 + j;
        if ((unsigned)k < (unsigned)n) {
            const float df = s[a + j] - s[k];
            d += df * df;
        }
    }
#pragma unroll
    for (int r = 0; r < NLM_RUN; ++r) {
        if (r < len) {
            const int t = t0 + r;
            if (t > 0 && t < n) {       // sample 0 is never a neighbour
                const float w = __builtin_amdgcn_exp2f(d * cexp);
                acc[r] = fmaf(w, s[t], acc[r]);
                z[r] += w;
            }
            if (r + 1 < len) {
                const int kn = t + p + 1, ko = t - p;
                float en = 0.f, eo = 0.f;
                if ((unsigned)kn < (unsigned)n) { const float df = s[a + r + p + 1] - s[kn]; en = df * df; }
                if ((unsigned)ko < (unsigned)n) { const float df = s[a + r - p] - s[ko]; eo = df * df; }
                d = (d + en) - eo;
            }
        }
    }
}

// NLM_U consecutive t0 (t0 >= NLM_P, t0 + NLM_U - 1 + NLM_RUN - 1 + NLM_P < n): every pair in bounds, every neighbour in (0, n)
__device__ __forceinline__ void nlm_fast(const float *s, int a, int t0, float cexp, const float (&xo)[NLM_WN], float (&acc)[NLM_RUN],
                                         float (&z)[NLM_RUN]) {
    float xs[NLM_WN + NLM_U - 1];
#pragma unroll
    for (int j = 0; j < NLM_WN + NLM_U - 1; ++j) xs[j] = s[t0 - NLM_P + j];
#pragma unroll
    for (int u = 0; u < NLM_U; ++u) {
        {
            float e[NLM_WN];
#pragma unroll
            for (int j = 0; j < NLM_WN; ++j) {
                const float df = xo[j] - xs[j + u];
                e[j] = df * df;
            }
            float d = e[0];
#pragma unroll
            for (int j = 1; j <= 2 * NLM_P; ++j) d += e[j];
#pragma unroll
            for (int r = 0; r < NLM_RUN; ++r) {
                const float w = __builtin_amdgcn_exp2f(d * cexp);
                acc[r] = fmaf(w, xs[u + NLM_P + r], acc[r]);
                z[r] += w;
                if (r + 1 < NLM_RUN) d = (d + e[r + 2 * NLM_P + 1]) - e[r];
            }
        }
    }
}

template <int CAP> __global__ __launch_bounds__(NLM_MAX_THREADS) void nlm_kernel(NlmArgs g) {
    __shared__ float s[CAP];
    const int rec = blockIdx.x, c = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int n = g.raw_len[rec];
    if (n <= 0 || n > CAP || n > g.max_len) return;
    const int64_t base = g.src_off[rec] + (int64_t)c * g.lead_stride;
    const float *__restrict__ x = g.x + base;
    float *out = g.out + base;
    for (int i = tid; i < n; i += nthr) s[i] = x[i];
    __syncthreads();           // from here on the lead is read from LDS alone: out may be x
    const int p = g.p, M = n - 2 * p - 1;      // output samples p + 1 .. n - p - 1
    const double sg = g.scale * g.sigma[(int64_t)rec * g.C + c];
    const double h = 2.0 * (double)(2 * p + 1) * sg * sg;
    const float cexp = (float)(-1.4426950408889634 / h);      // w = 2^(d cexp) = exp(-d / h)
    const bool through = M <= 0 || !(h > 0.0) || !(cexp - cexp == 0.f);
    const bool copy = out != x;
    if (through) {             // n <= 2p + 1, or sigma == 0 (the reference divides 0 by 0 there), or 1 / h past f32
        if (copy) for (int i = tid; i < n; i += nthr) out[i] = s[i];
        return;
    }
    if (copy) {
        for (int i = tid; i < p + 1; i += nthr) out[i] = s[i];
        for (int i = n - p + tid; i < n; i += nthr) out[i] = s[i];
    }
    const int W = g.W <= 0 || g.W > n ? n : g.W, W1 = W - 1;
    const int K = (M + NLM_RUN - 1) / NLM_RUN;
    const int len = M < NLM_RUN ? M : NLM_RUN;
    const bool fast = p == NLM_P && M >= NLM_RUN;
    const int f_lo = p, f_hi = n - NLM_RUN - p;        // t0 for which the whole neighbour window is in bounds
    for (int k = tid; k < K; k += nthr) {
        const int first = p + 1 + k * NLM_RUN;                         // the first sample this run stores
        const int a = k == K - 1 ? n - p - len : first;                // the last run ends on sample n - p - 1
        float acc[NLM_RUN], z[NLM_RUN], xo[NLM_WN];
#pragma unroll
        for (int r = 0; r < NLM_RUN; ++r) { acc[r] = 0.f; z[r] = 0.f; }
        if (fast) {
#pragma unroll
            for (int j = 0; j < NLM_WN; ++j) xo[j] = s[a - NLM_P + j];
        }
        // t0 - a is the shift: |t0 - a| <= W - 1.  Below 2 - len no neighbour t0 + r is past sample 0.  With the default W = n the range is the
        // same for every lane (a - W1 <= 1 - p - len); a narrower search makes it the lane's own, and costs in proportion to W
        int t0 = max(2 - len, a - W1);
        const int t_end = min(n - 1, a + W1);
        while (t0 <= t_end) {
            if (fast && t0 >= f_lo && t0 + NLM_U - 1 <= f_hi && t0 + NLM_U - 1 <= t_end) {
                nlm_fast(s, a, t0, cexp, xo, acc, z);
                t0 += NLM_U;
            } else {
                nlm_general(s, n, p, a, len, t0, cexp, acc, z);
                t0 += 1;
            }
        }
#pragma unroll
        for (int r = 0; r < NLM_RUN; ++r)
            if (r < len && a + r >= first) out[a + r] = acc[r] / (z[r] + 2.220446049250313e-16f);
    }
}

int ecgvit_nlm_denoise(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len,
                       const double *sigma, double scale, int patch_wd, int sch_wd, void *stream) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len) || !out || (reinterpret_cast<uintptr_t>(out) & 3u) || !sigma ||
        (reinterpret_cast<uintptr_t>(sigma) & 7u) || patch_wd < 1 || patch_wd > DN_MAX_LEN || sch_wd < 0 || !(scale > 0.0) || !(scale - scale == 0.0))
        return ECGVIT_EINVAL;
    NlmArgs g;
    g.x = x; g.out = out; g.src_off = src_off; g.lead_stride = lead_stride; g.raw_len = raw_len; g.sigma = sigma; g.scale = scale;
    g.C = C; g.p = patch_wd; g.W = sch_wd; g.max_len = max_len;
    // one lane per run of the longest record, whole waves, at most NLM_MAX_THREADS (a lane then takes several runs)
    const int M = max_len - 2 * patch_wd - 1;
    int runs = M > 0 ? (M + NLM_RUN - 1) / NLM_RUN : 1;
    int threads = (runs + WAVE - 1) / WAVE * WAVE;
    if (threads > NLM_MAX_THREADS) threads = NLM_MAX_THREADS;
    if (max_len <= 4096) hipLaunchKernelGGL(nlm_kernel<4096>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    else if (max_len <= 8192) hipLaunchKernelGGL(nlm_kernel<8192>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    else hipLaunchKernelGGL(nlm_kernel<DN_MAX_LEN>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
