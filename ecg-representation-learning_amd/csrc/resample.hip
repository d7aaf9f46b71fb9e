// Fourier resampling of a record store to another length (resample.py; the reference's preprocess/data_export.py:202-215 through
// wfdb.processing.resample_sig -> scipy.signal.resample).  include/ecgvit_hip.h states the algorithm in full: the spectrum rule, the lead pairing,
// the plan rule and the twiddle definition.  Complex f64 mixed-radix Stockham passes between two workspace buffers in global memory, one launch per
// pass for a whole group of records of one (n_in, n_out) pair, grid (butterfly blocks, record x lead pair).  No atomics, no device trigonometry:
// every root of unity is read from the two tables the caller passes.
#include "common.h"

#define RS_MAX_PASSES 32
#define RS_THREADS 256

typedef double2 cd;

__device__ __forceinline__ cd rs_mul(cd a, cd b) { return cd{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cd rs_add(cd a, cd b) { return cd{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd rs_sub(cd a, cd b) { return cd{a.x - b.x, a.y - b.y}; }

// the built radices, largest first; every other prime factor follows in ascending order, one generic pass each
static const int RS_BUILT[] = {25, 16, 8, 5, 4, 3, 2};

static int rs_plan(int n, int *radices, int cap) {
    if (n < 1 || n > ECGVIT_RESAMPLE_MAX_LEN || cap < 0 || (cap > 0 && !radices)) return -1;
    int cnt = 0;
    for (int r : RS_BUILT)
        while (n % r == 0) {
            if (cnt >= cap) return -1;
            radices[cnt++] = r;
            n /= r;
        }
    for (int p = 7; n > 1; p += 2) {
        if ((int64_t)p * p > n) p = n;          // what is left is a prime
        while (n % p == 0) {
            if (cnt >= cap) return -1;
            radices[cnt++] = p;
            n /= p;
        }
    }
    return cnt;
}

int ecgvit_resample_plan(int n, int *radices, int cap) { return rs_plan(n, radices, cap); }

static bool rs_is_built(int r) {
    for (int b : RS_BUILT)
        if (b == r) return true;
    return false;
}

// the plan of a length the launcher runs: every generic radix within ECGVIT_RESAMPLE_MAX_GENERIC
static int rs_plan_checked(int n, int *radices) {
    const int cnt = rs_plan(n, radices, RS_MAX_PASSES);
    for (int i = 0; i < cnt; ++i)
        if (!rs_is_built(radices[i]) && radices[i] > ECGVIT_RESAMPLE_MAX_GENERIC) return -1;
    return cnt;
}

static int64_t rs_workspace(int R, int C, int n_in, int n_out) {
    int rad[RS_MAX_PASSES];
    if (R <= 0 || C <= 0 || (C & 1) || C > 65534 || (int64_t)R * (C / 2) > ECGVIT_RESAMPLE_MAX_GRID_Y) return 0;
    if (rs_plan_checked(n_in, rad) < 0 || rs_plan_checked(n_out, rad) < 0) return 0;
    return 2 * 16 * (int64_t)R * (C / 2) * (int64_t)(n_in > n_out ? n_in : n_out);
}

int64_t ecgvit_resample_workspace(int R, int C, int n_in, int n_out) { return rs_workspace(R, C, n_in, n_out); }

// ---- the chirp route (Bluestein): a whole transform of length n as a circular convolution of length M, the smallest 2^a 3^b 5^c >= 2 n - 1 ------
static int rs_chirp_length(int n) {
    if (n < 1 || n > ECGVIT_RESAMPLE_MAX_CHIRP) return -1;
    const int64_t need = 2 * (int64_t)n - 1;
    int64_t best = (int64_t)ECGVIT_RESAMPLE_MAX_LEN;         // 2^25 >= 2 n - 1 for every admitted n
    for (int64_t p5 = 1; p5 <= best; p5 *= 5)
        for (int64_t p3 = p5; p3 <= best; p3 *= 3) {
            int64_t m = p3;
            while (m < need) m *= 2;
            if (m < best) best = m;
        }
    return (int)best;
}

int ecgvit_resample_chirp_length(int n) { return rs_chirp_length(n); }

// one side of a resample: the length the passes run at (n, or M on the chirp route) and their plan; false for what is refused
struct rs_side {
    int n, len, cnt, rad[RS_MAX_PASSES];
    bool chirp;
};

static bool rs_side_plan(int n, bool chirp, rs_side *s) {
    s->n = n;
    s->chirp = chirp;
    s->len = chirp ? rs_chirp_length(n) : n;
    if (s->len < 1) return false;
    s->cnt = rs_plan_checked(s->len, s->rad);
    return s->cnt >= 0;
}

static int64_t rs_chirp_workspace(int R, int C, int n_in, int n_out, int chirp_in, int chirp_out) {
    rs_side a, b;
    if (R <= 0 || C <= 0 || (C & 1) || C > 65534 || (int64_t)R * (C / 2) > ECGVIT_RESAMPLE_MAX_GRID_Y) return 0;
    if (!rs_side_plan(n_in, chirp_in != 0, &a) || !rs_side_plan(n_out, chirp_out != 0, &b)) return 0;
    return 2 * 16 * (int64_t)R * (C / 2) * (int64_t)(a.len > b.len ? a.len : b.len);
}

int64_t ecgvit_resample_chirp_workspace(int R, int C, int n_in, int n_out, int chirp_in, int chirp_out) {
    return rs_chirp_workspace(R, C, n_in, n_out, chirp_in, chirp_out);
}

// ---- pack: leads 2p, 2p + 1 of a record -> the real and imaginary parts of transform t = rec * P + p ------------------------------------------
__global__ __launch_bounds__(RS_THREADS) void rs_pack_kernel(const float *x, const int64_t *src_off, int64_t lead_stride, int P, int n, cd *buf) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int t = blockIdx.y, rec = t / P, p = t - rec * P;
    const float *a = x + src_off[rec] + (int64_t)(2 * p) * lead_stride;
    buf[(int64_t)t * n + i] = cd{(double)a[i], (double)a[lead_stride + i]};
}

__global__ __launch_bounds__(RS_THREADS) void rs_unpack_kernel(const cd *buf, float *out, const int64_t *dst_off, int64_t lead_stride, int P, int n) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int t = blockIdx.y, rec = t / P, p = t - rec * P;
    float *a = out + dst_off[rec] + (int64_t)(2 * p) * lead_stride;
    const cd v = buf[(int64_t)t * n + i];
    a[i] = (float)v.x;
    a[lead_stride + i] = (float)v.y;
}

// ---- the spectrum of n_in bins onto the grid of n_out bins (scipy.signal.resample, complex input), times 1 / n_in -------------------------------
__global__ __launch_bounds__(RS_THREADS) void rs_map_kernel(const cd *X, cd *Y, int n_in, int n_out, double scale) {
    const int m = blockIdx.x * RS_THREADS + threadIdx.x;
    if (m >= n_out) return;
    X += (int64_t)blockIdx.y * n_in;
    Y += (int64_t)blockIdx.y * n_out;
    const int N = n_in < n_out ? n_in : n_out, half = N / 2, nneg = N - (half + 1);
    cd v = cd{0.0, 0.0};
    if (m <= half) v = X[m];
    else if (m >= n_out - nneg) v = X[n_in - (n_out - m)];
    if ((N & 1) == 0) {
        if (n_out < n_in) {                     // downsampling: the bin at +N/2 takes the one at -N/2 too
            if (m == half) v = rs_add(v, X[n_in - half]);
        } else if (n_in < n_out) {              // upsampling: the bin at N/2 is halved and shared with -N/2
            if (m == half) v = cd{0.5 * v.x, 0.5 * v.y};
            else if (m == n_out - half) v = cd{0.5 * X[half].x, 0.5 * X[half].y};
        }
    }
    Y[m] = cd{v.x * scale, v.y * scale};
}

// ---- the chirp route's element-wise kernels: w the chirp table of the side (n entries), a transform of that side lives at stride M --------------
__device__ __forceinline__ cd rs_conj(cd a) { return cd{a.x, -a.y}; }
// post: D = DFT_M(conj(DFT_M(a) filter)) = conj(c) -> X[k] = w[k] conj(D[k])
__device__ __forceinline__ cd rs_chirp_post(cd D, cd w) { return rs_mul(w, rs_conj(D)); }

// pack with the chirp multiply and the zero fill folded in: a[j] = z[j] w[j], j < n; 0, n <= j < M
__global__ __launch_bounds__(RS_THREADS) void rs_pack_chirp_kernel(const float *x, const int64_t *src_off, int64_t lead_stride, int P, int n, int M,
                                                                    const cd *w, cd *buf) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= M) return;
    const int t = blockIdx.y, rec = t / P, p = t - rec * P;
    cd v = cd{0.0, 0.0};
    if (i < n) {
        const float *a = x + src_off[rec] + (int64_t)(2 * p) * lead_stride;
        v = rs_mul(cd{(double)a[i], (double)a[lead_stride + i]}, w[i]);
    }
    buf[(int64_t)t * M + i] = v;
}

// the pointwise product, conjugated, in place: A[j] <- conj(A[j] filter[j]), j < M
__global__ __launch_bounds__(RS_THREADS) void rs_chirp_mul_kernel(cd *A, const cd *filter, int M) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= M) return;
    cd *a = A + (int64_t)blockIdx.y * M + j;
    *a = rs_conj(rs_mul(*a, filter[j]));
}

// unpack with the post multiply folded in: y[k] = w[k] conj(D[k]), k < n, rounded once to f32
__global__ __launch_bounds__(RS_THREADS) void rs_unpack_chirp_kernel(const cd *buf, float *out, const int64_t *dst_off, int64_t lead_stride, int P, int n,
                                                                      int M, const cd *w) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int t = blockIdx.y, rec = t / P, p = t - rec * P;
    float *a = out + dst_off[rec] + (int64_t)(2 * p) * lead_stride;
    const cd v = rs_chirp_post(buf[(int64_t)t * M + i], w[i]);
    a[i] = (float)v.x;
    a[lead_stride + i] = (float)v.y;
}

// the spectrum map of rs_map_kernel with either chirp side folded in.  w_in != null: the input holds D at stride s_in and bin k is read as
// w_in[k] conj(D[k]) (post); else it holds X at stride s_in = n_in.  w_out != null: the output is the inverse side's operand at stride s_out = M:
// Y[m] scale w_out[m], m < n_out, and 0 for n_out <= m < M (pre, zero fill); else Y at stride s_out = n_out.
__global__ __launch_bounds__(RS_THREADS) void rs_map_chirp_kernel(const cd *X, cd *Y, int n_in, int n_out, int s_in, int s_out, double scale,
                                                                   const cd *w_in, const cd *w_out) {
    const int m = blockIdx.x * RS_THREADS + threadIdx.x;
    if (m >= s_out) return;
    X += (int64_t)blockIdx.y * s_in;
    Y += (int64_t)blockIdx.y * s_out;
    if (m >= n_out) {
        Y[m] = cd{0.0, 0.0};
        return;
    }
    auto bin = [&](int k) { return w_in ? rs_chirp_post(X[k], w_in[k]) : X[k]; };
    const int N = n_in < n_out ? n_in : n_out, half = N / 2, nneg = N - (half + 1);
    cd v = cd{0.0, 0.0};
    if (m <= half) v = bin(m);
    else if (m >= n_out - nneg) v = bin(n_in - (n_out - m));
    if ((N & 1) == 0) {
        if (n_out < n_in) {
            if (m == half) v = rs_add(v, bin(n_in - half));
        } else if (n_in < n_out) {
            if (m == half) v = cd{0.5 * v.x, 0.5 * v.y};
            else if (m == n_out - half) {
                const cd h = bin(half);
                v = cd{0.5 * h.x, 0.5 * h.y};
            }
        }
    }
    v = cd{v.x * scale, v.y * scale};
    Y[m] = w_out ? rs_mul(v, w_out[m]) : v;
}

// the filter of a length: b[j] = conj(w[j]), j < n; b[M - j] = conj(w[j]), 1 <= j < n; 0 elsewhere (M >= 2 n - 1: the two ranges do not meet)
__global__ __launch_bounds__(RS_THREADS) void rs_chirp_filter_kernel(const cd *w, cd *b, int n, int M) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= M) return;
    cd v = cd{0.0, 0.0};
    if (j < n) v = rs_conj(w[j]);
    else if (M - j < n) v = rs_conj(w[M - j]);
    b[j] = v;
}

__global__ __launch_bounds__(RS_THREADS) void rs_scale_kernel(const cd *in, cd *out, int M, double scale) {
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= M) return;
    out[j] = cd{in[j].x * scale, in[j].y * scale};
}

// ---- one Stockham pass of a built radix R = A * B, in registers -------------------------------------------------------------------------------
// Butterfly j < n / R, k = j % Ns (Ns: the product of the radices of the earlier passes): v[q] = in[j + q n / R] * tw[q k n / (Ns R)],
// u = DFT_R(v), out[(j - k) R + k + p Ns] = u[p].  DFT_R for B > 1 is the two-level form q = B q1 + q2, p = p1 + A p2:
// t[p1][q2] = sum_q1 v[B q1 + q2] w_A^(p1 q1), times w_R^(p1 q2), u[p1 + A p2] = sum_q2 t[p1][q2] w_B^(p2 q2); w_M^e = tw[e n / M].  A root with
// exponent 0 is not multiplied, one with exponent M / 2 is a negation; every other root is the table's value.  Sums run in ascending q.
template <int M> __device__ __forceinline__ cd rs_root_mul(cd v, int e, const cd (&w)[M]) {
    e %= M;
    if (e == 0) return v;
    if (2 * e == M) return cd{-v.x, -v.y};
    return rs_mul(v, w[e]);
}

template <int A, int B> __global__ __launch_bounds__(RS_THREADS) void rs_pass_kernel(const cd *in, cd *out, const cd *tw, int n, int Ns) {
    constexpr int R = A * B;
    const int m = n / R;
    const int j = blockIdx.x * RS_THREADS + threadIdx.x;
    if (j >= m) return;
    in += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * n;
    const int k = j % Ns;
    cd v[R];
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = in[j + q * m];
    if (k) {
        const int step = k * (m / Ns);          // q * step < n
#pragma unroll
        for (int q = 1; q < R; ++q) v[q] = rs_mul(v[q], tw[q * step]);
    }
    cd wA[A];
#pragma unroll
    for (int a = 0; a < A; ++a) wA[a] = tw[a * (n / A)];
    cd u[R];
    if constexpr (B == 1) {
#pragma unroll
        for (int p = 0; p < A; ++p) {
            cd s = v[0];
#pragma unroll
            for (int q = 1; q < A; ++q) s = rs_add(s, rs_root_mul<A>(v[q], p * q, wA));
            u[p] = s;
        }
    } else {
        cd wB[B], wR[(A - 1) * (B - 1) + 1];
#pragma unroll
        for (int b = 0; b < B; ++b) wB[b] = tw[b * (n / B)];
#pragma unroll
        for (int e = 0; e <= (A - 1) * (B - 1); ++e) wR[e] = tw[e * m];
        cd t[A][B];
#pragma unroll
        for (int q2 = 0; q2 < B; ++q2)
#pragma unroll
            for (int p1 = 0; p1 < A; ++p1) {
                cd s = v[q2];
#pragma unroll
                for (int q1 = 1; q1 < A; ++q1) s = rs_add(s, rs_root_mul<A>(v[B * q1 + q2], p1 * q1, wA));
                t[p1][q2] = (p1 * q2) ? rs_mul(s, wR[p1 * q2]) : s;
            }
#pragma unroll
        for (int p1 = 0; p1 < A; ++p1)
#pragma unroll
            for (int p2 = 0; p2 < B; ++p2) {
                cd s = t[p1][0];
#pragma unroll
                for (int q2 = 1; q2 < B; ++q2) s = rs_add(s, rs_root_mul<B>(t[p1][q2], p2 * q2, wB));
                u[p1 + A * p2] = s;
            }
    }
    cd *o = out + (int64_t)(j - k) * R + k;
#pragma unroll
    for (int p = 0; p < R; ++p) o[(int64_t)p * Ns] = u[p];
}

// ---- one Stockham pass of any radix r: a thread per output, a loop over the r inputs ---------------------------------------------------------
// Output o = (j - k) r + k + p Ns: out[o] = sum_q in[j + q n / r] * tw[(q * e) % n], e = (o % (Ns r)) * (n / (Ns r)) -- the pass's twiddle and the
// root of DFT_r in one table entry -- in ascending q.  r == n (Ns == 1) is the dense DFT.
__global__ __launch_bounds__(RS_THREADS) void rs_generic_kernel(const cd *in, cd *out, const cd *tw, int n, int Ns, int r) {
    const int64_t o64 = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (o64 >= n) return;
    const int o = (int)o64;
    in += (int64_t)blockIdx.y * n;
    out += (int64_t)blockIdx.y * n;
    const int64_t span = (int64_t)Ns * r;       // <= n
    const int rem = (int)(o % span), blk = (int)(o / span), k = rem % Ns;
    const int j = blk * Ns + k, m = n / r;
    const int e = rem * (int)(n / span);        // < n
    int t = 0;
    cd s = cd{0.0, 0.0};
    for (int q = 0; q < r; ++q) {
        s = rs_add(s, rs_mul(in[j + (int64_t)q * m], tw[t]));
        t += e;
        if (t >= n) t -= n;
    }
    out[o] = s;
}

// the passes of one length over T transforms: cur -> other, swapped after each -> the buffer that holds the result
static cd *rs_run_passes(cd *cur, cd *other, const cd *tw, int n, int T, const int *rad, int cnt, hipStream_t st) {
    int Ns = 1;
    for (int i = 0; i < cnt; ++i) {
        const int r = rad[i];
        const dim3 block(RS_THREADS);
        const dim3 grid((unsigned)((n / r + RS_THREADS - 1) / RS_THREADS), T);
        switch (rs_is_built(r) ? r : 0) {
        case 25: hipLaunchKernelGGL((rs_pass_kernel<5, 5>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 16: hipLaunchKernelGGL((rs_pass_kernel<4, 4>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 8: hipLaunchKernelGGL((rs_pass_kernel<4, 2>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 5: hipLaunchKernelGGL((rs_pass_kernel<5, 1>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 4: hipLaunchKernelGGL((rs_pass_kernel<4, 1>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 3: hipLaunchKernelGGL((rs_pass_kernel<3, 1>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        case 2: hipLaunchKernelGGL((rs_pass_kernel<2, 1>), grid, block, 0, st, cur, other, tw, n, Ns); break;
        default:
            hipLaunchKernelGGL(rs_generic_kernel, dim3((unsigned)((n + RS_THREADS - 1) / RS_THREADS), T), block, 0, st, cur, other, tw, n, Ns, r);
        }
        cd *tmp = cur; cur = other; other = tmp;
        Ns *= r;
    }
    return cur;
}

// the chirp convolution of T operands a (stride M, chirp-multiplied and zero-filled) in `cur`: DFT_M, the pointwise product with the filter
// (conjugated, in place), DFT_M again -> the buffer that holds D = conj(c)
static cd *rs_run_chirp(cd *cur, cd *other, const cd *tw, const cd *filter, const rs_side &s, int T, hipStream_t st) {
    cd *res = rs_run_passes(cur, other, tw, s.len, T, s.rad, s.cnt, st);
    cd *spare = res == cur ? other : cur;
    hipLaunchKernelGGL(rs_chirp_mul_kernel, dim3((unsigned)((s.len + RS_THREADS - 1) / RS_THREADS), T), dim3(RS_THREADS), 0, st, res, filter, s.len);
    return rs_run_passes(res, spare, tw, s.len, T, s.rad, s.cnt, st);
}

static bool rs_misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int ecgvit_resample(const float *x, float *out, const int64_t *src_off, int64_t src_stride, const int64_t *dst_off, int64_t dst_stride, int R, int C,
                    int n_in, int n_out, const double *tw_in, const double *tw_out, void *workspace, void *stream) {
    if (!x || !out || !src_off || !dst_off || !tw_in || !tw_out || !workspace || src_stride <= 0 || dst_stride <= 0) return ECGVIT_EINVAL;
    if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u) || (reinterpret_cast<uintptr_t>(src_off) & 7u) ||
        (reinterpret_cast<uintptr_t>(dst_off) & 7u) || (reinterpret_cast<uintptr_t>(tw_in) & 15u) || (reinterpret_cast<uintptr_t>(tw_out) & 15u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return ECGVIT_EINVAL;
    if (rs_workspace(R, C, n_in, n_out) <= 0) return ECGVIT_EINVAL;
    int rad_in[RS_MAX_PASSES], rad_out[RS_MAX_PASSES];
    const int cnt_in = rs_plan_checked(n_in, rad_in), cnt_out = rs_plan_checked(n_out, rad_out);
    if (cnt_in < 0 || cnt_out < 0) return ECGVIT_EINVAL;
    const int P = C / 2, T = R * P;
    const int64_t nmax = n_in > n_out ? n_in : n_out;
    cd *a = reinterpret_cast<cd *>(workspace), *b = a + (int64_t)T * nmax;
    hipStream_t st = as_stream(stream);
    const dim3 block(RS_THREADS), grid_in((unsigned)((n_in + RS_THREADS - 1) / RS_THREADS), T), grid_out((unsigned)((n_out + RS_THREADS - 1) / RS_THREADS), T);
    hipLaunchKernelGGL(rs_pack_kernel, grid_in, block, 0, st, x, src_off, src_stride, P, n_in, a);
    cd *cur = rs_run_passes(a, b, reinterpret_cast<const cd *>(tw_in), n_in, T, rad_in, cnt_in, st);
    cd *other = cur == a ? b : a;
    hipLaunchKernelGGL(rs_map_kernel, grid_out, block, 0, st, cur, other, n_in, n_out, 1.0 / (double)n_in);
    cur = rs_run_passes(other, cur, reinterpret_cast<const cd *>(tw_out), n_out, T, rad_out, cnt_out, st);
    hipLaunchKernelGGL(rs_unpack_kernel, grid_out, block, 0, st, cur, out, dst_off, dst_stride, P, n_out);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_resample_chirp_filter(const double *chirp, int n, int M, const double *tw_M, double *filter, void *workspace, void *stream) {
    if (!chirp || !tw_M || !filter || !workspace) return ECGVIT_EINVAL;
    if (rs_misaligned(chirp, 15u) || rs_misaligned(tw_M, 15u) || rs_misaligned(filter, 15u) || rs_misaligned(workspace, 15u)) return ECGVIT_EINVAL;
    rs_side s;
    if (!rs_side_plan(n, true, &s) || s.len != M) return ECGVIT_EINVAL;
    cd *a = reinterpret_cast<cd *>(workspace), *b = a + M;
    hipStream_t st = as_stream(stream);
    const dim3 block(RS_THREADS), grid((unsigned)((M + RS_THREADS - 1) / RS_THREADS));
    hipLaunchKernelGGL(rs_chirp_filter_kernel, grid, block, 0, st, reinterpret_cast<const cd *>(chirp), a, n, M);
    const cd *B = rs_run_passes(a, b, reinterpret_cast<const cd *>(tw_M), M, 1, s.rad, s.cnt, st);
    hipLaunchKernelGGL(rs_scale_kernel, grid, block, 0, st, B, reinterpret_cast<cd *>(filter), M, 1.0 / (double)M);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

int ecgvit_resample_chirp(const float *x, float *out, const int64_t *src_off, int64_t src_stride, const int64_t *dst_off, int64_t dst_stride, int R,
                          int C, int n_in, int n_out, const double *tw_in, const double *tw_out, const double *chirp_in, const double *filter_in,
                          const double *chirp_out, const double *filter_out, void *workspace, void *stream) {
    if (!x || !out || !src_off || !dst_off || !tw_in || !tw_out || !workspace || src_stride <= 0 || dst_stride <= 0) return ECGVIT_EINVAL;
    if (!chirp_in != !filter_in || !chirp_out != !filter_out) return ECGVIT_EINVAL;      // a chirp table and a filter come as a pair
    if (rs_misaligned(x, 3u) || rs_misaligned(out, 3u) || rs_misaligned(src_off, 7u) || rs_misaligned(dst_off, 7u) || rs_misaligned(tw_in, 15u) ||
        rs_misaligned(tw_out, 15u) || rs_misaligned(chirp_in, 15u) || rs_misaligned(filter_in, 15u) || rs_misaligned(chirp_out, 15u) ||
        rs_misaligned(filter_out, 15u) || rs_misaligned(workspace, 15u))
        return ECGVIT_EINVAL;
    if (rs_chirp_workspace(R, C, n_in, n_out, chirp_in != nullptr, chirp_out != nullptr) <= 0) return ECGVIT_EINVAL;
    if (!chirp_in && !chirp_out)                // both sides plain: ecgvit_resample's launches, its bits
        return ecgvit_resample(x, out, src_off, src_stride, dst_off, dst_stride, R, C, n_in, n_out, tw_in, tw_out, workspace, stream);
    rs_side si, so;
    if (!rs_side_plan(n_in, chirp_in != nullptr, &si) || !rs_side_plan(n_out, chirp_out != nullptr, &so)) return ECGVIT_EINVAL;
    const int P = C / 2, T = R * P;
    const int64_t lmax = si.len > so.len ? si.len : so.len;
    cd *a = reinterpret_cast<cd *>(workspace), *b = a + (int64_t)T * lmax;
    const cd *twi = reinterpret_cast<const cd *>(tw_in), *two = reinterpret_cast<const cd *>(tw_out);
    const cd *wi = reinterpret_cast<const cd *>(chirp_in), *wo = reinterpret_cast<const cd *>(chirp_out);
    hipStream_t st = as_stream(stream);
    const dim3 block(RS_THREADS);
    auto grid = [T](int len) { return dim3((unsigned)((len + RS_THREADS - 1) / RS_THREADS), T); };
    cd *cur;
    if (si.chirp) {
        hipLaunchKernelGGL(rs_pack_chirp_kernel, grid(si.len), block, 0, st, x, src_off, src_stride, P, n_in, si.len, wi, a);
        cur = rs_run_chirp(a, b, twi, reinterpret_cast<const cd *>(filter_in), si, T, st);
    } else {
        hipLaunchKernelGGL(rs_pack_kernel, grid(n_in), block, 0, st, x, src_off, src_stride, P, n_in, a);
        cur = rs_run_passes(a, b, twi, n_in, T, si.rad, si.cnt, st);
    }
    cd *other = cur == a ? b : a;
    hipLaunchKernelGGL(rs_map_chirp_kernel, grid(so.len), block, 0, st, cur, other, n_in, n_out, si.len, so.len, 1.0 / (double)n_in, wi, wo);
    if (so.chirp) {
        cur = rs_run_chirp(other, cur, two, reinterpret_cast<const cd *>(filter_out), so, T, st);
        hipLaunchKernelGGL(rs_unpack_chirp_kernel, grid(n_out), block, 0, st, cur, out, dst_off, dst_stride, P, n_out, so.len, wo);
    } else {
        cur = rs_run_passes(other, cur, two, n_out, T, so.rad, so.cnt, st);
        hipLaunchKernelGGL(rs_unpack_kernel, grid(n_out), block, 0, st, cur, out, dst_off, dst_stride, P, n_out);
    }
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}

#ifdef ECGVIT_TOOLS
// tools/ecgvit_hip_tools.h: ONE pass of radix r (after passes of product Ns) over T transforms of length n, in -> out, as ecgvit_resample
// launches it: what tools/resample_rate.py times per pass kind
extern "C" int ecgvit_tools_resample_pass(const void *in, void *out, const double *tw, int n, int T, int Ns, int r, void *stream) {
    if (!in || !out || in == out || !tw || n < 1 || n > ECGVIT_RESAMPLE_MAX_LEN || T < 1 || T > ECGVIT_RESAMPLE_MAX_GRID_Y || r < 2 || Ns < 1 || n % r || (n / r) % Ns) return ECGVIT_EINVAL;
    if (!rs_is_built(r) && r > ECGVIT_RESAMPLE_MAX_GENERIC) return ECGVIT_EINVAL;
    rs_run_passes(reinterpret_cast<cd *>(const_cast<void *>(in)), reinterpret_cast<cd *>(out), reinterpret_cast<const cd *>(tw), n, T, &r, 1, as_stream(stream));
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
// the chirp route's two stand-alone ends: complex f64 in (stride n) -> the operand a (stride M); D (stride M) -> complex f64 out (stride n)
__global__ __launch_bounds__(RS_THREADS) void rs_tools_chirp_pre_kernel(const cd *in, cd *buf, int n, int M, const cd *w) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= M) return;
    buf[(int64_t)blockIdx.y * M + i] = i < n ? rs_mul(in[(int64_t)blockIdx.y * n + i], w[i]) : cd{0.0, 0.0};
}

__global__ __launch_bounds__(RS_THREADS) void rs_tools_chirp_post_kernel(const cd *buf, cd *out, int n, int M, const cd *w) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    out[(int64_t)blockIdx.y * n + i] = rs_chirp_post(buf[(int64_t)blockIdx.y * M + i], w[i]);
}

// tools/ecgvit_hip_tools.h: the chirp DFT of T complex f64 sequences of length n, in complex f64 (the product's passes, pointwise product and
// post multiply; the pre multiply as a kernel of its own)
extern "C" int ecgvit_tools_resample_chirp(const void *in, void *out, const double *chirp, const double *filter, const double *tw_M, int n, int M, int T,
                                           void *workspace, void *stream) {
    if (!in || !out || !chirp || !filter || !tw_M || !workspace || T < 1 || T > ECGVIT_RESAMPLE_MAX_GRID_Y) return ECGVIT_EINVAL;
    rs_side s;
    if (!rs_side_plan(n, true, &s) || s.len != M) return ECGVIT_EINVAL;
    cd *a = reinterpret_cast<cd *>(workspace), *b = a + (int64_t)T * M;
    const cd *w = reinterpret_cast<const cd *>(chirp);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(rs_tools_chirp_pre_kernel, dim3((unsigned)((M + RS_THREADS - 1) / RS_THREADS), T), dim3(RS_THREADS), 0, st,
                       reinterpret_cast<const cd *>(in), a, n, M, w);
    const cd *D = rs_run_chirp(a, b, reinterpret_cast<const cd *>(tw_M), reinterpret_cast<const cd *>(filter), s, T, st);
    hipLaunchKernelGGL(rs_tools_chirp_post_kernel, dim3((unsigned)((n + RS_THREADS - 1) / RS_THREADS), T), dim3(RS_THREADS), 0, st, D,
                       reinterpret_cast<cd *>(out), n, M, w);
    ECGVIT_CHECK_LAUNCH();
    return ECGVIT_OK;
}
#endif
