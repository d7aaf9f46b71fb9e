// The Zheng et al. denoiser (denoise.py; the reference's preprocess/data_preprocessor.py): zero-phase low-pass, the noise estimate and non-local
// means, per (record, lead), over a record store addressed as fit_stats.hip addresses it.  Contracts and the order of every sum: include/ecgvit_hip.h.
//
// One workgroup per (record, lead) in every kernel but the two tiled along time for records past ECGVIT_DENOISE_MAX_LEN (nlm_tiled_kernel, rloess_tiled_kernel:
// grid (record, lead, tile), each described where it stands).  The robust LOESS baseline (rloess_kernel) is described at the end of the file.
// Of the other three:  The low-pass and the noise estimate are sequential recurrences in f64: lane 0 walks
// them chunk by chunk through LDS while the whole workgroup moves the chunks (coalesced), and their f64 intermediates live in a caller's
// workspace.  Non-local means is the hot path: the lead sits in LDS as f32, a lane owns runs of NLM_RUN consecutive output samples.
#include "common.h"

#define DN_WS_PAD 64                // workspace doubles per lead beyond max_len (the low-pass's two extensions: 2 * 3 * 9 = 54)
#define DN_MAX_TAPS ECGVIT_DENOISE_MAX_TAPS

static bool dn_store_ok(const float *x, const int64_t *src_off, const int32_t *raw_len, int R, int C, int max_len, int cap = ECGVIT_DENOISE_MAX_LEN) {
    return x && src_off && raw_len && R > 0 && C > 0 && C <= 65535 && max_len > 0 && max_len <= cap && (reinterpret_cast<uintptr_t>(x) & 3u) == 0 &&
           (reinterpret_cast<uintptr_t>(src_off) & 7u) == 0 && (reinterpret_cast<uintptr_t>(raw_len) & 3u) == 0;
}

static int64_t dn_workspace(int R, int C, int max_len, int cap) {
    if (R <= 0 || C <= 0 || max_len <= 0 || max_len > cap) return 0;
    return (int64_t)R * C * (max_len + DN_WS_PAD) * 8;
}
int64_t ecgvit_denoise_workspace(int R, int C, int max_len) { return dn_workspace(R, C, max_len, ECGVIT_DENOISE_MAX_LEN); }
int64_t ecgvit_denoise_workspace_long(int R, int C, int max_len) { return dn_workspace(R, C, max_len, ECGVIT_DENOISE_MAX_LEN_TILED); }

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

// both entry points: the same kernel, so a record's bits are the same from either; only the cap of max_len differs
static int ff_launch(int cap, const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                     int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len, cap) || !out || (reinterpret_cast<uintptr_t>(out) & 3u) || !workspace ||
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

int ecgvit_filtfilt(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                    int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream) {
    return ff_launch(ECGVIT_DENOISE_MAX_LEN, x, out, src_off, lead_stride, raw_len, R, C, min_len, max_len, b, a, zi, ntaps, workspace, stream);
}
int ecgvit_filtfilt_long(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                         int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream) {
    return ff_launch(ECGVIT_DENOISE_MAX_LEN_TILED, x, out, src_off, lead_stride, raw_len, R, C, min_len, max_len, b, a, zi, ntaps, workspace, stream);
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

static int sg_launch(int cap, const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                     void *workspace, void *stream) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len, cap) || !sigma || (reinterpret_cast<uintptr_t>(sigma) & 7u) || !workspace ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u))
        return ECGVIT_EINVAL;
    hipLaunchKernelGGL(nlm_sigma_kernel, dim3(R, C), dim3(SG_THREADS), 0, as_stream(stream), x, src_off, lead_stride, raw_len, C, max_len, sigma,
                       reinterpret_cast<double *>(workspace));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_nlm_sigma(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                     void *workspace, void *stream) {
    return sg_launch(ECGVIT_DENOISE_MAX_LEN, x, src_off, lead_stride, raw_len, R, C, max_len, sigma, workspace, stream);
}
int ecgvit_nlm_sigma_long(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                          void *workspace, void *stream) {
    return sg_launch(ECGVIT_DENOISE_MAX_LEN_TILED, x, src_off, lead_stride, raw_len, R, C, max_len, sigma, workspace, stream);
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
#define NLM_RUN ECGVIT_DENOISE_NLM_RUN
#define NLM_P 10
#define NLM_U 1                     // t0 per neighbour-window load of the fast body: 1 keeps the kernel at 158 VGPRs, three waves per SIMD (4: 256)
#define NLM_WN (NLM_RUN + 2 * NLM_P)
#define NLM_MAX_THREADS ECGVIT_DENOISE_NLM_MAX_THREADS

struct NlmArgs {
    const float *x;
    float *out;
    const int64_t *src_off;
    int64_t lead_stride;
    const int32_t *raw_len;
    const double *sigma;
    double scale;
    int C, p, W, max_len;
    int tile_runs;              // nlm_tiled_kernel alone: runs per workgroup
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
// win: the neighbour window's first sample, s + t0 - NLM_P
__device__ __forceinline__ void nlm_fast(const float *win, float cexp, const float (&xo)[NLM_WN], float (&acc)[NLM_RUN], float (&z)[NLM_RUN]) {
    float xs[NLM_WN + NLM_U - 1];
#pragma unroll
    for (int j = 0; j < NLM_WN + NLM_U - 1; ++j) xs[j] = win[j];
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
                nlm_fast(s + (t0 - NLM_P), cexp, xo, acc, z);
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

// the checks and the arguments both launchers share -> false when the call is refused
static bool nlm_args(NlmArgs &g, int cap, const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C,
                     int max_len, const double *sigma, double scale, int patch_wd, int sch_wd) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len, cap) || !out || (reinterpret_cast<uintptr_t>(out) & 3u) || !sigma ||
        (reinterpret_cast<uintptr_t>(sigma) & 7u) || patch_wd < 1 || patch_wd > cap || sch_wd < 0 || !(scale > 0.0) || !(scale - scale == 0.0))
        return false;
    g.x = x; g.out = out; g.src_off = src_off; g.lead_stride = lead_stride; g.raw_len = raw_len; g.sigma = sigma; g.scale = scale;
    g.C = C; g.p = patch_wd; g.W = sch_wd; g.max_len = max_len; g.tile_runs = 0;
    return true;
}

int ecgvit_nlm_denoise(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len,
                       const double *sigma, double scale, int patch_wd, int sch_wd, void *stream) {
    NlmArgs g;
    if (!nlm_args(g, ECGVIT_DENOISE_MAX_LEN, x, out, src_off, lead_stride, raw_len, R, C, max_len, sigma, scale, patch_wd, sch_wd)) return ECGVIT_EINVAL;
    // one lane per run of the longest record, whole waves, at most NLM_MAX_THREADS (a lane then takes several runs)
    const int M = max_len - 2 * patch_wd - 1;
    int runs = M > 0 ? (M + NLM_RUN - 1) / NLM_RUN : 1;
    int threads = (runs + WAVE - 1) / WAVE * WAVE;
    if (threads > NLM_MAX_THREADS) threads = NLM_MAX_THREADS;
    if (max_len <= 4096) hipLaunchKernelGGL(nlm_kernel<4096>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    else if (max_len <= 8192) hipLaunchKernelGGL(nlm_kernel<8192>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    else hipLaunchKernelGGL(nlm_kernel<ECGVIT_DENOISE_MAX_LEN>, dim3(R, C), dim3(threads), 0, as_stream(stream), g);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

// -----------------------------------------------------------------------------------------------------
// non-local means, tiled along time: grid (record, lead, tile), a workgroup owns tile_runs consecutive runs of one lead and nothing keeps the
// whole lead on the CU.  The run decomposition and the order of every sum are nlm_kernel's (the same two bodies), so the bits are its bits.
// A lane's own window comes from global memory into registers; the neighbour side of the fast body is streamed: the workgroup walks the hull of
// its lanes' t0 ranges in ascending chunks of NLT_CHUNK, stages x[t0c - P .. t0c + NLT_CHUNK + RUN - 1 + P) into one of two LDS buffers while it
// computes on the other, and a lane takes the t0 of the chunk that lie in its own range (the full search: the same for every lane, so the
// window stays one LDS broadcast).  The general body (any patch_wd, t0 near either end) reads global memory: x is not written by this launch
// (the launcher refuses out == x); it walks the same chunks, so that both bodies keep one call site as in nlm_kernel, and stages nothing where
// no lane takes the fast body.  Every barrier sits in loops whose bounds are uniform across the workgroup.
// -----------------------------------------------------------------------------------------------------
#define NLT_CHUNK 256
#define NLT_SPAN (NLT_CHUNK + NLM_RUN - 1 + 2 * NLM_P)

__global__ __launch_bounds__(NLM_MAX_THREADS) void nlm_tiled_kernel(NlmArgs g) {
    __shared__ float sb[2][NLT_SPAN];
    const int rec = blockIdx.x, c = blockIdx.y, tile = blockIdx.z, tid = threadIdx.x, nthr = blockDim.x;
    const int n = g.raw_len[rec];
    if (n <= 0 || n > g.max_len) return;
    const int64_t base = g.src_off[rec] + (int64_t)c * g.lead_stride;
    const float *__restrict__ x = g.x + base;
    float *__restrict__ out = g.out + base;
    const int p = g.p, M = n - 2 * p - 1;      // output samples p + 1 .. n - p - 1
    const double sg = g.scale * g.sigma[(int64_t)rec * g.C + c];
    const double h = 2.0 * (double)(2 * p + 1) * sg * sg;
    const float cexp = (float)(-1.4426950408889634 / h);
    if (M <= 0 || !(h > 0.0) || !(cexp - cexp == 0.f)) {          // copied through: every tile of the launch takes a share
        for (int i = tile * nthr + tid; i < n; i += (int)gridDim.z * nthr) out[i] = x[i];
        return;
    }
    if (tile == 0) {
        for (int i = tid; i < p + 1; i += nthr) out[i] = x[i];
        for (int i = n - p + tid; i < n; i += nthr) out[i] = x[i];
    }
    const int W = g.W <= 0 || g.W > n ? n : g.W, W1 = W - 1;
    const int K = (M + NLM_RUN - 1) / NLM_RUN;
    const int len = M < NLM_RUN ? M : NLM_RUN;
    const int f_hi = p == NLM_P && M >= NLM_RUN ? n - NLM_RUN - NLM_P : -1;    // the fast body's t0 are NLM_P .. f_hi; -1: none (nlm_kernel's !fast)
    const int k0 = tile * g.tile_runs;
    if (k0 >= K) return;                       // a tile past this record's last run: before the first barrier
    const int k1 = min(K, k0 + g.tile_runs);
    for (int kp = k0; kp < k1; kp += nthr) {   // uniform: lane tid takes run kp + tid of each pass
        const int k = kp + tid;
        const bool live = k < k1;
        const int first = p + 1 + k * NLM_RUN;
        const int a = k == K - 1 ? n - p - len : first;
        float acc[NLM_RUN], z[NLM_RUN], xo[NLM_WN];
#pragma unroll
        for (int r = 0; r < NLM_RUN; ++r) { acc[r] = 0.f; z[r] = 0.f; }
        if (f_hi >= 0) {
#pragma unroll
            for (int j = 0; j < NLM_WN; ++j) xo[j] = live ? x[a - NLM_P + j] : 0.f;
        }
        const int lo = live ? max(2 - len, a - W1) : 1, hi = live ? min(n - 1, a + W1) : 0;      // the lane's own t0, as in nlm_kernel
        // the hull of the pass's ranges: a grows with the run, so the first lane has the lowest and the last live lane the highest t0
        const int kl = min(k1, kp + nthr) - 1;
        const int a_f = kp == K - 1 ? n - p - len : p + 1 + kp * NLM_RUN, a_l = kl == K - 1 ? n - p - len : p + 1 + kl * NLM_RUN;
        const int h_lo = max(2 - len, a_f - W1), h_hi = min(n - 1, a_l + W1);
        const int nch = (h_hi - h_lo) / NLT_CHUNK + 1;              // (h_hi >= h_lo: a_f is an output sample)
        if (f_hi >= 0)
            for (int i = tid; i < NLT_SPAN; i += nthr) { const int gi = h_lo - NLM_P + i; sb[0][i] = (unsigned)gi < (unsigned)n ? x[gi] : 0.f; }
        __syncthreads();
        for (int ci = 0; ci < nch; ++ci) {
            const int t0c = h_lo + ci * NLT_CHUNK;
            if (f_hi >= 0 && ci + 1 < nch)          // the next chunk into the other buffer: its last readers passed the barrier below
                for (int i = tid; i < NLT_SPAN; i += nthr) {
                    const int gi = t0c + NLT_CHUNK - NLM_P + i;
                    sb[(ci + 1) & 1][i] = (unsigned)gi < (unsigned)n ? x[gi] : 0.f;
                }
            const float *w = sb[ci & 1];
            const int u_hi = min(hi, t0c + NLT_CHUNK - 1);
            for (int t0 = max(lo, t0c); t0 <= u_hi; ++t0) {
                if (t0 >= NLM_P && t0 <= f_hi) nlm_fast(w + (t0 - t0c), cexp, xo, acc, z);
                else nlm_general(x, n, p, a, len, t0, cexp, acc, z);
            }
            __syncthreads();
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < NLM_RUN; ++r)
                if (r < len && a + r >= first) out[a + r] = acc[r] / (z[r] + 2.220446049250313e-16f);
        }
    }
}

int ecgvit_nlm_denoise_tiled(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len,
                             const double *sigma, double scale, int patch_wd, int sch_wd, int tile_runs, void *stream) {
    NlmArgs g;
    if (tile_runs < 0 || !nlm_args(g, ECGVIT_DENOISE_MAX_LEN_TILED, x, out, src_off, lead_stride, raw_len, R, C, max_len, sigma, scale, patch_wd, sch_wd))
        return ECGVIT_EINVAL;
    if (out == x) return ECGVIT_EINVAL;        // a workgroup reads samples that another one writes
    const int64_t M = (int64_t)max_len - 2 * (int64_t)patch_wd - 1;
    const int runs = M > 0 ? (int)((M + NLM_RUN - 1) / NLM_RUN) : 1;
    g.tile_runs = min(tile_runs == 0 ? NLM_MAX_THREADS : tile_runs, runs);
    const int tiles = (runs + g.tile_runs - 1) / g.tile_runs;
    if (tiles > ECGVIT_DENOISE_MAX_TILES) return ECGVIT_EINVAL;
    int threads = (g.tile_runs + WAVE - 1) / WAVE * WAVE;
    if (threads > NLM_MAX_THREADS) threads = NLM_MAX_THREADS;
    hipLaunchKernelGGL(nlm_tiled_kernel, dim3(R, C, tiles), dim3(threads), 0, as_stream(stream), g);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

// =====================================================================================================
// robust LOESS baseline (the reference's rloess: loess_1d(x, sig, degree=2, npoints=n)[1] of the `loess` package, which is not available: the
// algorithm is the one include/ecgvit_hip.h states in full, and parity with the package is UNPINNED).  Two choices are made here where the
// reference leaves the result open: for an even window the two samples at distance m / 2 tie and the LOWER index enters the window (the
// reference's unstable argsort takes either, by numpy version and CPU); a window whose median absolute residual is 0 (below the smallest normal
// f64) ends its robust loop and keeps the fit it has (the reference divides by zero).
//
// One workgroup per (record, lead), the lead in LDS as f32; one wave per output sample j, window sample lo + lane + 64 v in slot v of the lane
// (NV = ceil(m / 64) slots: distance weight, residual and the f32 sample in registers).  f64 throughout, without contraction into fma: every
// operation is the IEEE one in the order written, which tests/loess_ref.py restates operation for operation.
//   fit      eight moment sums (S_k = sum w s^k, k = 0 .. 4; T_k = sum w s^k y, k = 0 .. 2; s = (i - j) (1 / d)): a lane adds its slots in
//            ascending order from +0, the wave adds lanes by the xor butterfly 32, 16, .. 1; a slot past the window adds +0, so the sums do not
//            depend on NV.  The (g + 1) x (g + 1) normal equations are solved by elimination without pivoting (symmetric positive definite in
//            the scaled abscissa); the value at j is the constant coefficient.
//   median   exact: the non-negative f64 patterns order as integers; the k-th smallest is found bit by bit from bit 62, counting the samples
//            below the trial value with one wave ballot per slot (scalar population counts: no cross-lane sums), until one candidate is left.
// =====================================================================================================
#pragma clang fp contract(off)
#define RL_THREADS 512
#define RL_CUT 0.34
#define RL_MIN_MAD 2.2250738585072014e-308

struct RloessArgs {
    const float *x;
    float *out;
    const int64_t *src_off;
    int64_t lead_stride;
    const int32_t *raw_len;
    int8_t *iters;
    double frac;
    int C, max_len, npoints, degree, robust_iters, subtract;
    int tile_samples;           // rloess_tiled_kernel alone: output samples per workgroup
};

// the reference's force_odd(int(n * frac) - 1), as Python computes it: truncation of the f64 product, floor division by 2
__host__ __device__ __forceinline__ int rl_frac_points(int n, double frac) {
    const int k = (int)((double)n * frac) - 1;
    return 2 * (k >= 0 ? k / 2 : -((1 - k) / 2)) + 1;
}

__device__ __forceinline__ double rl_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long rl_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

template <int NV> struct RlWindow {
    double dw[NV], aerr[NV];     // distance weight (0 past the window), |fit - y| of the last fit (+inf past the window)
    float y[NV];
    int t0;                      // (lo + lane) - j: slot v holds the window sample at signed distance t0 + 64 v
    double inv_d;
};

// weighted fit with weights dw * bw, bw = (1 - min((aerr inv6)^2, 1))^2 (inv6 == 0: bw = 1, the distance-weighted fit).  -> the coefficients
// (every lane holds them) and the lane's outlier bits (bw < 0.34, one per slot); a slot past the window has bw = 0 in every robust fit
template <int NV> __device__ __forceinline__ unsigned rl_fit(const RlWindow<NV> &w, double inv6, int degree, double &a0, double &a1, double &a2) {
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, S3 = 0.0, S4 = 0.0, T0 = 0.0, T1 = 0.0, T2 = 0.0;
    unsigned bad = 0u;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double s = (double)(w.t0 + 64 * v) * w.inv_d;
        const double q = w.aerr[v] * inv6;
        const double u = 1.0 - fmin(q * q, 1.0);
        const double bw = u * u;
        bad |= (bw < RL_CUT ? 1u : 0u) << v;
        const double wt = w.dw[v] * bw, y = (double)w.y[v];
        const double w1 = wt * s, w2 = w1 * s, w3 = w2 * s, w4 = w3 * s;
        S0 += wt; S1 += w1; S2 += w2; S3 += w3; S4 += w4;
        T0 += wt * y; T1 += w1 * y; T2 += w2 * y;
    }
    S0 = rl_wave_sum(S0); S1 = rl_wave_sum(S1); S2 = rl_wave_sum(S2); T0 = rl_wave_sum(T0); T1 = rl_wave_sum(T1);
    const double r0 = 1.0 / S0;
    const double l1 = S1 * r0;
    const double A11 = S2 - l1 * S1, B1 = T1 - l1 * T0;
    if (degree == 2) {
        S3 = rl_wave_sum(S3); S4 = rl_wave_sum(S4); T2 = rl_wave_sum(T2);
        const double l2 = S2 * r0;
        const double A12 = S3 - l1 * S2, A22 = S4 - l2 * S2, B2 = T2 - l2 * T0;
        const double r1 = 1.0 / A11;
        const double l21 = A12 * r1;
        const double D22 = A22 - l21 * A12, E2 = B2 - l21 * B1;
        a2 = E2 / D22;
        a1 = (B1 - A12 * a2) * r1;
        a0 = ((T0 - S1 * a1) - S2 * a2) * r0;
    } else {
        a2 = 0.0;
        a1 = B1 / A11;
        a0 = (T0 - S1 * a1) * r0;
    }
    return bad;
}

template <int NV> __device__ __forceinline__ void rl_residuals(RlWindow<NV> &w, int m, int lane, double a0, double a1, double a2) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const double s = (double)(w.t0 + 64 * v) * w.inv_d;
        const double f = a0 + s * (a1 + s * a2);
        w.aerr[v] = lane + 64 * v < m ? fabs(f - (double)w.y[v]) : __builtin_huge_val();
    }
}

// np.median of the window's residuals: the (m - 1) / 2-th smallest, for even m its mean with the next one.  Wave-uniform control flow.
template <int NV> __device__ __forceinline__ double rl_median(const RlWindow<NV> &w, int m) {
    unsigned long long key[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) key[v] = (unsigned long long)__double_as_longlong(w.aerr[v]);     // +inf past the window: above every sample
    const int k = (m - 1) / 2;
    unsigned long long prefix = 0ull;
    int below = 0, cand = m, b = 62;
    for (; b >= 0 && cand > 1; --b) {
        const unsigned long long mid = prefix | (1ull << b);
        int cnt = 0;
#pragma unroll
        for (int v = 0; v < NV; ++v) cnt += __popcll(__ballot(key[v] < mid));
        if (k < cnt) {
            cand = cnt - below;
        } else {
            prefix = mid;
            cand = below + cand - cnt;
            below = cnt;
        }
    }
    // the candidates are the keys in [prefix, prefix + 2^(b + 1)): one key, or equal ones
    const unsigned long long span = b >= 0 ? (2ull << b) - 1ull : 0ull;
    unsigned long long best = 0ull;
#pragma unroll
    for (int v = 0; v < NV; ++v) best = (key[v] >= prefix && key[v] - prefix <= span && key[v] > best) ? key[v] : best;
    const unsigned long long k1 = rl_wave_max(best);
    if (m & 1) return __longlong_as_double((long long)k1);
    int le = 0;
    unsigned long long next = ~0ull;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        le += __popcll(__ballot(key[v] <= k1));
        next = (key[v] > k1 && key[v] < next) ? key[v] : next;
    }
    unsigned long long k2 = k1;
    if (le <= k + 1) k2 = ~rl_wave_max(~next);
    return (__longlong_as_double((long long)k1) + __longlong_as_double((long long)k2)) / 2.0;
}

// one output sample by one wave: window placement, the distance-weighted fit, the robust loop.  s[i - sb] holds sample i of the lead for every i
// of the window.  -> the fit's value at j (every lane holds it); it: the robust iterations run
template <int NV> __device__ __forceinline__ double rl_sample(const float *s, int sb, int n, int m, int half, int j, int lane, int degree, int robust_iters,
                                                              int &it) {
    const int lo = min(max(j - half, 0), n - m);
    const int d = max(j - lo, lo + m - 1 - j);
    RlWindow<NV> w;
    w.t0 = lo + lane - j;
    w.inv_d = 1.0 / (double)d;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const bool in = lane + 64 * v < m;
        const double a = fabs((double)(w.t0 + 64 * v) * w.inv_d);
        const double u = 1.0 - a * a * a;
        w.dw[v] = in ? u * u * u : 0.0;
        w.y[v] = in ? s[lo + lane + 64 * v - sb] : 0.f;
        w.aerr[v] = 0.0;
    }
    double a0, a1, a2;
    rl_fit<NV>(w, 0.0, degree, a0, a1, a2);
    unsigned bad = 0u;
    it = 0;
    while (it < robust_iters) {
        rl_residuals<NV>(w, m, lane, a0, a1, a2);
        const double mad = rl_median<NV>(w, m);
        if (!(mad >= RL_MIN_MAD)) break;
        const unsigned now = rl_fit<NV>(w, 1.0 / (6.0 * mad), degree, a0, a1, a2);
        const bool same = it > 0 && __ballot(now != bad) == 0ull;
        bad = now;
        ++it;
        if (same) break;
    }
    return a0;
}

template <int NV, int CAP> __global__ __launch_bounds__(RL_THREADS) void rloess_kernel(RloessArgs g) {
    __shared__ float s[CAP];
    const int rec = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int n = g.raw_len[rec];
    if (n <= 0 || n > CAP || n > g.max_len) return;
    int m = g.frac > 0.0 ? rl_frac_points(n, g.frac) : g.npoints;
    if (m > n) m = n;
    if (m < g.degree + 2 || m > 64 * NV) return;         // (the launcher refused both for the lengths the caller promised)
    const int64_t base = g.src_off[rec] + (int64_t)c * g.lead_stride;
    const float *x = g.x + base;       // (no __restrict__: out may be x)
    float *out = g.out + base;
    for (int i = tid; i < n; i += RL_THREADS) s[i] = x[i];
    __syncthreads();           // from here on the lead is read from LDS alone: out may be x
    int8_t *iters = g.iters ? g.iters + ((int64_t)rec * g.C + c) * g.max_len : nullptr;
    const int lane = tid & 63, half = (m & 1) ? (m - 1) / 2 : m / 2;
    for (int j = tid >> 6; j < n; j += RL_THREADS / 64) {
        int it;
        const double a0 = rl_sample<NV>(s, 0, n, m, half, j, lane, g.degree, g.robust_iters, it);
        if (lane == 0) {
            out[j] = g.subtract ? (float)((double)s[j] - a0) : (float)a0;
            if (iters) iters[j] = (int8_t)it;
        }
    }
}

// tiled along time: grid (record, lead, tile), a workgroup owns tile_samples consecutive output samples and keeps them with one window of halo on
// either side in LDS: x[max(0, j0 - m) .. min(n, j0 + tile_samples + m)).  A sample's arithmetic reads only its window and is rl_sample's, so the
// output and the iteration counts are rloess_kernel's bit for bit.  Other workgroups write out while this one reads x: the launcher refuses out == x.
#define RLT_TILE (ECGVIT_DENOISE_LOESS_LDS - 2 * ECGVIT_DENOISE_MAX_POINTS)

template <int NV> __global__ __launch_bounds__(RL_THREADS) void rloess_tiled_kernel(RloessArgs g) {
    __shared__ float s[ECGVIT_DENOISE_LOESS_LDS];
    const int rec = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int n = g.raw_len[rec];
    if (n <= 0 || n > g.max_len) return;
    int m = g.frac > 0.0 ? rl_frac_points(n, g.frac) : g.npoints;
    if (m > n) m = n;
    if (m < g.degree + 2 || m > 64 * NV) return;
    const int j0 = (int)blockIdx.z * g.tile_samples;
    if (j0 >= n) return;               // a tile past this record's end: before the barrier
    const int j1 = min(n, j0 + g.tile_samples);
    const int s0 = max(0, j0 - m), s1 = min(n, j0 + g.tile_samples + m);
    if (s1 - s0 > ECGVIT_DENOISE_LOESS_LDS) return;     // (the launcher refused a tile that does not fit with the widest window)
    const int64_t base = g.src_off[rec] + (int64_t)c * g.lead_stride;
    const float *x = g.x + base;
    float *out = g.out + base;
    for (int i = s0 + tid; i < s1; i += RL_THREADS) s[i - s0] = x[i];
    __syncthreads();
    int8_t *iters = g.iters ? g.iters + ((int64_t)rec * g.C + c) * g.max_len : nullptr;
    const int lane = tid & 63, half = (m & 1) ? (m - 1) / 2 : m / 2;
    for (int j = j0 + (tid >> 6); j < j1; j += RL_THREADS / 64) {
        int it;
        const double a0 = rl_sample<NV>(s, s0, n, m, half, j, lane, g.degree, g.robust_iters, it);
        if (lane == 0) {
            out[j] = g.subtract ? (float)((double)s[j - s0] - a0) : (float)a0;
            if (iters) iters[j] = (int8_t)it;
        }
    }
}

// the one NV dispatch: launch(NV) with the slots a lane needs for the widest window, as a compile-time constant: 1, 2, 4, 8 or 16
template <class F> static void rl_dispatch(int nv, F launch) {
    if (nv <= 1) launch(std::integral_constant<int, 1>());
    else if (nv <= 2) launch(std::integral_constant<int, 2>());
    else if (nv <= 4) launch(std::integral_constant<int, 4>());
    else if (nv <= 8) launch(std::integral_constant<int, 8>());
    else launch(std::integral_constant<int, 16>());
}

// the checks and the arguments both launchers share -> the widest window of the launch, or 0 when the call is refused
static int rl_args(RloessArgs &g, int cap, const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C,
                   int min_len, int max_len, int npoints, double frac, int degree, int robust_iters, int subtract, int8_t *iters) {
    if (!dn_store_ok(x, src_off, raw_len, R, C, max_len, cap) || !out || (reinterpret_cast<uintptr_t>(out) & 3u) || lead_stride <= 0) return 0;
    if (degree < 1 || degree > 2 || robust_iters < 0 || robust_iters > ECGVIT_DENOISE_MAX_ROBUST_ITERS || (subtract != 0 && subtract != 1)) return 0;
    if (!(frac >= 0.0 && frac <= 1.0) || min_len < degree + 2 || min_len > max_len) return 0;
    int widest = npoints;
    if (frac > 0.0) {          // the window of the shortest and of the longest record: a fraction's width grows with the length
        widest = rl_frac_points(max_len, frac);
        if (rl_frac_points(min_len, frac) < degree + 2) return 0;
    }
    if (widest < degree + 2 || widest > ECGVIT_DENOISE_MAX_POINTS) return 0;
    g.x = x; g.out = out; g.src_off = src_off; g.lead_stride = lead_stride; g.raw_len = raw_len; g.iters = iters; g.frac = frac;
    g.C = C; g.max_len = max_len; g.npoints = npoints; g.degree = degree; g.robust_iters = robust_iters; g.subtract = subtract; g.tile_samples = 0;
    return min(widest, max_len);
}

int ecgvit_rloess(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                  int max_len, int npoints, double frac, int degree, int robust_iters, int subtract, int8_t *iters, void *stream) {
    RloessArgs g;
    const int widest = rl_args(g, ECGVIT_DENOISE_MAX_LEN, x, out, src_off, lead_stride, raw_len, R, C, min_len, max_len, npoints, frac, degree, robust_iters, subtract,
                               iters);
    if (widest <= 0) return ECGVIT_EINVAL;
    const int nv = (widest + 63) / 64;
    const dim3 grid(R, C), block(RL_THREADS);
    hipStream_t st = as_stream(stream);
    if (max_len <= 8192) rl_dispatch(nv, [&](auto v) { hipLaunchKernelGGL((rloess_kernel<decltype(v)::value, 8192>), grid, block, 0, st, g); });
    else rl_dispatch(nv, [&](auto v) { hipLaunchKernelGGL((rloess_kernel<decltype(v)::value, ECGVIT_DENOISE_MAX_LEN>), grid, block, 0, st, g); });
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_rloess_tiled(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                        int max_len, int npoints, double frac, int degree, int robust_iters, int subtract, int8_t *iters, int tile_samples,
                        void *stream) {
    RloessArgs g;
    const int widest = rl_args(g, ECGVIT_DENOISE_MAX_LEN_TILED, x, out, src_off, lead_stride, raw_len, R, C, min_len, max_len, npoints, frac, degree, robust_iters,
                               subtract, iters);
    if (widest <= 0 || tile_samples < 0) return ECGVIT_EINVAL;
    if (out == x) return ECGVIT_EINVAL;        // a workgroup reads samples that another one writes
    g.tile_samples = tile_samples == 0 ? RLT_TILE : tile_samples;
    if (g.tile_samples > ECGVIT_DENOISE_LOESS_LDS || g.tile_samples + 2 * widest > ECGVIT_DENOISE_LOESS_LDS) return ECGVIT_EINVAL;
    const int tiles = (max_len + g.tile_samples - 1) / g.tile_samples;
    if (tiles > ECGVIT_DENOISE_MAX_TILES) return ECGVIT_EINVAL;
    const dim3 grid(R, C, tiles), block(RL_THREADS);
    hipStream_t st = as_stream(stream);
    rl_dispatch((widest + 63) / 64, [&](auto v) { hipLaunchKernelGGL(rloess_tiled_kernel<decltype(v)::value>, grid, block, 0, st, g); });
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
