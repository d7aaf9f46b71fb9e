/* Entry points of the TOOLS library only (ecg-representation-learning_amd/csrc/build/libecgvit_hip_tools.so = the product objects plus the
 * -DECGVIT_TOOLS builds of the kernel files; `make -C ecg-representation-learning_amd/csrc tools`).  Nothing here is part of the product
 * C-ABI (include/ecgvit_hip.h) or of the shipped library: probes that pin hardware fragment layouts for the tests, a second independent
 * implementation of the attention backward, the A/B switches of tools/*.py. */
#ifndef ECGVIT_HIP_TOOLS_H
#define ECGVIT_HIP_TOOLS_H
#include "../include/ecgvit_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* exact-integer dump of what each lane receives from the LDS fragment helpers and of the MFMA C layout (tests/test_gpu_ops.py) */
int ecgvit_probe_mfma_layout(float *out /* [4][64][16] */, void *stream);

/* The attention backward on the one-(record, head)-per-workgroup kernel (N <= 256; what ecgvit_attention_bwd itself runs for N <= 128):
 * an independent implementation of the same function, so that tests can hold the persistent kernel against it. */
int ecgvit_attention_bwd_oneitem(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv,
                                 int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, int dtype,
                                 void *stream);

/* forward: -1 (default) the product's dispatch; 0: always the one-item-per-workgroup forward; 1 / 2: always the streamed forward (round 6) --
 * up to 256 tokens in its two short-record forms (1: MODE 2, 2: MODE 3) */
int ecgvit_tools_attn_fwd_variant(int v);

/* one A . B^T call with column groups of raster_g n-tiles (0 = the built-in order): kernel 2 = gemm_nt_kernel's dispatch, 3 = gemm_nt_kernel_4w,
 * anything else = ecgvit_gemm (tools/gemm_ab.py) */
int ecgvit_tools_gemm(const ecgvit_gemm_desc *d, void *stream, int kernel, int raster_g);

/* one Stockham pass of ecgvit_resample alone: radix r after passes of product Ns, over T transforms of length n (complex f64, transform t at
 * element t * n), in -> out (in != out), tw the table of n roots the passes of that length read; r divides n and Ns divides n / r
 * (tools/resample_rate.py: the time per pass kind) */
int ecgvit_tools_resample_pass(const void *in, void *out, const double *tw, int n, int T, int Ns, int r, void *stream);

/* the chirp route of ecgvit_resample_chirp as a transform of its own, before the f32 store hides its f64 arithmetic: T complex f64 sequences of
 * length n (sequence t at element t * n of `in`) -> their DFT of the chirp table's sign, complex f64, in `out` (same layout).  chirp, filter,
 * tw_M, M as ecgvit_resample_chirp_filter states them; `workspace`: 2 T M complex f64.  The passes, the pointwise product and the post multiply
 * are the product's; the chirp multiply and zero fill of the operand is a kernel of its own here (tests/test_gpu_resample_chirp.py) */
int ecgvit_tools_resample_chirp(const void *in, void *out, const double *chirp, const double *filter, const double *tw_M, int n, int M, int T,
                                void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif
