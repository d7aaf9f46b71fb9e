/*
 * ecgvit_hip.h -- C-ABI of libecgvit_hip.so: the MI355X (gfx950) kernels behind the ECG-ViT train step.
 *
 * The reference (StefanHeng/ECG-Representation-Learning) has NO FFI / operator registry for this path:
 * its boundary is the Python class surface `EcgVitConfig` / `EcgVit.forward` (ecg_transformer/models/
 * ecg_vit.py:26-149) and the train-step body (ecg_transformer/models/train.py:268-283), and every
 * numeric op below is one the reference reaches through third-party `vit-pytorch==0.33.2` -> `torch.nn`
 * (reference call sites cited per entry point).  This header is therefore the build's own design for
 * what sits UNDER that Python surface; `INTEGRATION.md` shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless named `h_*`.
 *   - the caller owns every buffer (PyTorch caching allocator in the shipped host code); kernels never
 *     allocate, never synchronise, keep no global state, and are stream-ordered on `stream`
 *     (a `hipStream_t` passed as `void*`; NULL = the legacy default stream).
 *   - return 0 on success; ECGVIT_EINVAL for an unsupported shape/argument (nothing launched);
 *     ECGVIT_ELAUNCH if hipGetLastError() reported a launch failure.  Nothing throws across the ABI.
 *   - `dtype` selects the ACTIVATION element type: ECGVIT_F32 (parity path, exact-f32 MFMA / VALU) or
 *     ECGVIT_BF16 (throughput path, bf16 MFMA with f32 accumulate).  Parameters, gradients, optimiser
 *     state, LayerNorm statistics, logits and losses are always f32.
 *   - row-major everywhere; `ld*` are leading dimensions in ELEMENTS.
 */
#ifndef ECGVIT_HIP_H
#define ECGVIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECGVIT_OK 0
#define ECGVIT_EINVAL 1
#define ECGVIT_ELAUNCH 2

#define ECGVIT_F32 0
#define ECGVIT_BF16 1
#define ECGVIT_FP8_E4M3 2 /* OCP e4m3fn, 1 byte: GEMM operands only (ecgvit_gemm A/B, ecgvit_fp8_*)   */
#define ECGVIT_BF8_E5M2 3 /* OCP e5m2,   1 byte: the A operand of input-gradient products            */

/* library / build identification: "ecgvit-hip gfx950 <abi-version>" */
const char *ecgvit_version(void);
int ecgvit_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * GEMM: C[M,N] = epilogue( alpha * op(A) . op(B) )            (f32 accumulate)
 * replaces: nn.Linear forward/backward reached from vit_pytorch Attention.to_qkv / to_out / FeedForward.net
 * (reference ecg_vit.py:141 -> ViT.forward) and, in the f32 parity path, the batched QK^T / PV products.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_GEMM_NT 0 /* A[M,K] row-major, B[N,K] row-major :  C = A . B^T   (Linear forward)      */
#define ECGVIT_GEMM_NN 1 /* A[M,K] row-major, B[K,N] row-major :  C = A . B     (Linear input grad)   */
#define ECGVIT_GEMM_TN 2 /* A[K,M] row-major, B[K,N] row-major :  C = A^T . B   (Linear weight grad)  */

/* epilogue flags; applied in this order to v = alpha * acc */
#define ECGVIT_EPI_BIAS 1       /* v += bias[n]                                    (f32 bias)        */
#define ECGVIT_EPI_GELU 2       /* aux[m,n] = v ; v = gelu_erf(v)                  (exact erf GELU)  */
#define ECGVIT_EPI_GELU_BWD 4   /* v *= gelu_erf'(aux[m,n])                                          */
#define ECGVIT_EPI_RESIDUAL 8   /* v += residual[m,n]                                                */
#define ECGVIT_EPI_ACCUM 16     /* v += C[m,n]   (read-modify-write of the output)                   */
#define ECGVIT_EPI_DROPOUT 32   /* v = keep(seed, m*N+n) ? v / (1-p') : 0 ; applied after GELU / GELU_BWD,
                                   before RESIDUAL (the mask is a pure function of (seed, element)).  bf16 outputs: one hash per four
                                   consecutive elements, 8 bits each: p' = round(256 p) / 256 (0 < p < 1/512: ECGVIT_EINVAL); f32 outputs:
                                   one hash per pair, 16 bits each: p' = p.  The same rule holds for every dropout_p of this header
                                   (ecgvit_embed_finish / _bwd, ecgvit_layernorm_bwd_fused, ecgvit_dropout_apply): by element type        */
#define ECGVIT_EPI_GELU_GRAD_AUX 128 /* modifies EPI_GELU: aux[m,n] = gelu_erf'(v) * (the EPI_DROPOUT multiplier of this element, if any)
                                   instead of v -- everything the backward of `dropout(gelu(.))` needs, so that the input-gradient GEMM
                                   of the next Linear finishes with EPI_MUL_AUX alone (no erf, no mask hash in the backward)    */
#define ECGVIT_EPI_MUL_AUX 256  /* v *= aux[m,n]                                                                              */
#define ECGVIT_EPI_QUANT_OUT 512 /* additionally q8_out[m,n] = saturate(C[m,n] as stored / *q8_scale) in q8_format (ECGVIT_FP8_E4M3 | ECGVIT_BF8_E5M2),
                                   *q8_amax = max(*q8_amax, max |C| as stored): the 8-bit copy the next Linear's product consumes, written
                                   by the producer instead of by a separate quantise pass (8-bit A.B^T launches only)                        */
#define ECGVIT_EPI_NO_OUT 1024  /* with ECGVIT_EPI_QUANT_OUT, on the two FFN-wide emitting bodies of the 8-bit A.B^T kernel (BIAS|GELU|GELU_GRAD_AUX[|DROPOUT] and
                                   MUL_AUX|COLSUM): C is NOT written (C may be NULL) -- q8_out, *q8_amax, aux and colsum_out are exactly what the same
                                   call without the flag produces (of the bf16-rounded values C would have held).  For a consumer chain that reads
                                   only the 8-bit copy: 128 KiB less to store per 256 x 256 tile (ABI 5)                                       */
#define ECGVIT_EPI_AUX8 2048    /* modifies GELU_GRAD_AUX (bf16 products) and MUL_AUX: the saved tensor gelu'(v) x dropout multiplier is stored / read as e4m3 BYTES
                                   [M, ldaux] (ldaux in bytes) instead of bf16 (ABI 6): the tensor is private to the FFN-up forward and the FFN-down input gradient,
                                   790 MB per layer at 128 512 x 3072 whose HBM stream costs each of the two launches ~85 us (tools/gemm_ab.py --aux-ld0); values
                                   in [-0.14, 1.13] / (1 - p): three mantissa bits, relative error <= 2^-4 per element, unbiased.  Large A.B^T kernel only
                                   (ecgvit_gemm_kernel() == ECGVIT_KERNEL_GEMM_NT for the same descriptor), flag sets BIAS|GELU|GELU_GRAD_AUX[|DROPOUT] and
                                   MUL_AUX|COLSUM (8-bit operands: also with QUANT_OUT [|NO_OUT]); anything else: ECGVIT_EINVAL                                                                          */
#define ECGVIT_EPI_COLSUM 64    /* additionally colsum_out[n] = sum_m C[m,n] (of the values as stored): the bias gradient of
                                   the Linear whose output gradient this GEMM produces. Needs `workspace` of at least
                                   max(ecgvit_colsum_workspace(M,N), 8*ceil(M/256)*N) bytes. Deterministic two-stage sum. */

typedef struct ecgvit_gemm_desc {
    int32_t layout;    /* ECGVIT_GEMM_*                                             */
    int32_t dtype;     /* element type of A and B: ECGVIT_F32 | ECGVIT_BF16; or ECGVIT_FP8_E4M3 | ECGVIT_BF8_E5M2 = the 8-bit
                          format of A with B in e4m3: ECGVIT_GEMM_NT (K % 128 == 0, lda/ldb % 16 == 0, bf16 output), or ECGVIT_GEMM_TN
                          = weight gradients dW = dY8^T . X8 (M, N % 256 == 0, K >= 4096, lda/ldb % 16 == 0, f32 output, bias / accumulate
                          epilogues only; scale_a * scale_b is applied to the sum) */
    int32_t out_dtype; /* element type of C, aux, residual                          */
    int32_t epilogue;  /* OR of ECGVIT_EPI_*                                        */
    int32_t M, N, K;
    int32_t batch1, batch2; /* batched problems: z = z1 * batch2 + z2 (both >= 1)   */
    const void *A; int64_t lda, strideA1, strideA2;
    const void *B; int64_t ldb, strideB1, strideB2;
    void *C;       int64_t ldc, strideC1, strideC2;
    const float *bias;                    /* [N] f32                                 */
    const void *residual; int64_t ldr;    /* [M,N] out_dtype (not batched)           */
    void *aux;            int64_t ldaux;  /* [M,N] out_dtype (not batched)           */
    float alpha;
    float dropout_p;      /* in [0,1)                                                */
    uint64_t dropout_seed;
    void *workspace;      /* optional split-K slabs (bf16 TN); see ecgvit_gemm_workspace */
    int64_t workspace_bytes;
    float *colsum_out;    /* [N] f32, with ECGVIT_EPI_COLSUM */
    int32_t tiles_per_workgroup; /* large A.B^T products (gemm_nt launches) only. 0: persistent launch, one workgroup per CU walks a
                             static share of the output tiles (fastest when the launch owns the GPU). k > 0: ceil(tiles / k) workgroups
                             of about k tiles each, handed out by the hardware dispatcher as CUs free up -- use it when other kernels
                             (RCCL collectives overlapped with the backward pass) hold CUs, where a static share would leave the
                             workgroups that start late a full share behind. Results are bit-identical either way. Weight-gradient
                             (ECGVIT_GEMM_TN) products ignore the field: their K-slicing and sum order never depend on it. */
    void *q8_out; int64_t ldq8; const float *q8_scale; float *q8_amax; int32_t q8_format; /* with ECGVIT_EPI_QUANT_OUT */
    const float *scale_a, *scale_b; /* optional device scalars multiplied into alpha: the per-tensor scales of 8-bit operands
                             (x ~= q * scale), read by the kernel -- no host round trip between the quantise pass and the product */
} ecgvit_gemm_desc;

int ecgvit_gemm(const ecgvit_gemm_desc *d, void *stream);
/* Same product; every dropout epilogue draws the bits of output row m * mask_row_pitch (element index (m * mask_row_pitch) * N + n): a product
 * over one row per record (addressed compactly or through lda / ldc) applies exactly the mask the full launch applies to those rows.
 * mask_row_pitch >= 1; 1 == ecgvit_gemm. */
int ecgvit_gemm_rowpitch(const ecgvit_gemm_desc *d, int mask_row_pitch, void *stream);
/* which kernel family ecgvit_gemm would launch for this descriptor (nothing is launched, pointers are not dereferenced but must be
 * the real ones: alignment decides eligibility).  Lets a profiler attribute a call to a kernel symbol without restating the dispatch. */
#define ECGVIT_KERNEL_NONE 0        /* the call would return ECGVIT_EINVAL                                   */
#define ECGVIT_KERNEL_GEMM_F32 1    /* gemm_f32_kernel: exact-f32 MFMA parity path                           */
#define ECGVIT_KERNEL_GEMM_BF16 2   /* gemm_bf16_kernel: small / ragged bf16 products                        */
#define ECGVIT_KERNEL_GEMM_NT 3     /* gemm_nt_kernel / gemm_nt_kernel_4w (its four-wave body: plain K >= 1536, bias + residual K >= 768): persistent 256x256x64 A.B^T (bf16 or 8-bit operands) */
#define ECGVIT_KERNEL_GEMM_WGRAD 4  /* gemm_wgrad_kernel_4w / gemm_wgrad8_kernel_4w: streaming split-K weight gradients (four-wave bodies) */
int ecgvit_gemm_kernel(const ecgvit_gemm_desc *d);
/* bytes of workspace with which the call would use its preferred split-K factor (0 = none needed) */
int64_t ecgvit_gemm_workspace(const ecgvit_gemm_desc *d);

/* ------------------------------------------------------------------------------------------------
 * fp8 operand path (BASELINE.json configs[4]; nothing in the reference: its live trainer is f32, models/train.py:197).
 * Segment form: table[2s] = first element, table[2s+1] = element count of segment s inside x / y (multiples of 8), scale / amax
 * indexed by s; table == NULL with nseg == 1 means the single segment [0, count).  `count` = the longest segment.
 * ------------------------------------------------------------------------------------------------ */
/* amax[s] = max(amax[s], max |x|) over bf16 x */
int ecgvit_fp8_amax(const void *x, const int64_t *table, int nseg, int64_t count, float *amax, void *stream);
/* y = saturate(x / scale[s]) in `format` (ECGVIT_FP8_E4M3 | ECGVIT_BF8_E5M2), one byte per element at the same element offsets;
 * amax_next (optional) accumulates max |x| per segment for the next step's scale (delayed scaling).  Round to nearest even of x times the f32
 * reciprocal of scale[s], +-inf and everything beyond +-max give +-max, a scale that is not positive gives zeros.  NaN input is outside the
 * contract of every 8-bit emitter of this header: they clamp with a median and take the amax with fmaxf, neither of which propagates it */
int ecgvit_fp8_quantize(const void *x, void *y, const int64_t *table, int nseg, int64_t count, int format, const float *scale,
                        float *amax_next, void *stream);
/* scale[i] = amax[i] / FORMAT_MAX where amax[i] > 0 (else kept; 1.0 if never set); amax[i] = 0.  formats: per-entry, or NULL = format_all */
int ecgvit_fp8_scale_update(float *scale, float *amax, int n, const int32_t *formats, int format_all, void *stream);

/* ------------------------------------------------------------------------------------------------
 * patch embedding front end.  replaces: einops Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)')
 * inside vit_pytorch ViT.to_patch_embedding (reference ecg_vit.py:141, shape probe :277).
 * ------------------------------------------------------------------------------------------------ */
/* patches[(b*n + p) * ld + j*C + c] = x[b][c][p*P + j]; columns [C*P, ld) are zero-filled. x is f32. */
int ecgvit_patch_gather(const float *x, void *patches, int B, int C, int L, int P, int64_t ld, int dtype, void *stream);
/* Same gather with the reference's input transforms fused into the load (next row f2; preprocess/transform.py:18-35 Normalize,
 * :140-154 TimeEndPad, :175-185 TimeOut; wired at preprocess/ptb_dataset.py:132-149): x_raw is (B, C, L_raw) f32,
 * value(b,c,s) = s < L_raw and s not in [timeout_start[b], +timeout_len[b]) ? (x_raw - mean[c]) * inv_std[c] : 0, for s < L = n*P.
 * timeout_start / timeout_len: int32 [B] or both NULL (eval: no TimeOut). */
int ecgvit_patch_gather_transform(const float *x_raw, void *patches, int B, int C, int L_raw, int L, int P, int64_t ld,
                                  const float *mean, const float *inv_std, const int32_t *timeout_start,
                                  const int32_t *timeout_len, int dtype, void *stream);
/* The fused transforms PER RECORD, for records of unequal raw length -- what the reference does to one record at a time on the host
 * (preprocess/ptb_dataset.py:132-149: Normalize, TimeEndPad(patch_size), TimeOut; preprocess/transform.py:18-35, :140-154, :175-185).
 * Record b: raw_len[b] samples per lead, lead c at x + src_off[b] + c * lead_stride (lead_stride = W of a padded (B, C, W) batch with
 * src_off[b] = b C W, or S_raw of a ragged (C, S_raw) batch with src_off[b] = the raw sample offset); normalised, zero-padded in
 * normalised space to n_patch[b] * P samples, samples [timeout_start[b], + timeout_len[b]) of the padded record zeroed; its patch rows
 * are rows row_off[b] .. of `patches`.  n_rows_per_record = 0: packed rows, record b writes n_patch[b] rows; > 0 (>= n_max): padded rows,
 * record b writes that many, exact zeros past n_patch[b].  n_max >= every n_patch[b] (sizes the launch; a larger table entry is clamped).
 * Samples at or past raw_len[b] are never read.  Tables: device pointers, [B]; timeout_*: both NULL (eval) or both set. */
int ecgvit_patch_gather_transform_varlen(const float *x, void *patches, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len,
                                         const int32_t *n_patch, const int32_t *row_off, int n_rows_per_record, int n_max, int B, int C, int P,
                                         int64_t ld, const float *mean, const float *inv_std, const int32_t *timeout_start,
                                         const int32_t *timeout_len, int dtype, void *stream);
/* Same gather for variable-length records (attention_varlen.hip): n_tok int32 [B] on the device; patch p of record b is gathered for
 * p < n_tok[b] - 1 and zero past it (the samples there are never read). */
int ecgvit_patch_gather_varlen(const float *x, void *patches, const int32_t *n_tok, int B, int C, int L, int P, int64_t ld, int dtype,
                               void *stream);
/* X[b*N + 0] = cls + pos[0];  X[b*N + 1 + p] = tok[b*n + p] + pos[1 + p]   (N = n + 1; ViT.forward: cat CLS, += pos)
 * optional embedding dropout (p = emb_dropout_p, mask = f(seed, element index in X)). cls/pos are f32. */
int ecgvit_embed_finish(const void *tok, const float *cls, const float *pos, void *X, int B, int n, int d,
                        float dropout_p, uint64_t seed, int dtype, void *stream);
/* backward of embed_finish: dtok[b*n+p] = dX[b*N+1+p] ; dpos[t] = sum_b dX[b*N+t] ; dcls = sum_b dX[b*N] (f32 grads, overwritten) */
int ecgvit_embed_bwd(const void *dX, void *dtok, float *dcls, float *dpos, int B, int n, int d,
                     float dropout_p, uint64_t seed, int dtype, void *stream);
/* Ragged batch (records packed along the token rows, no padding): record b's tokens are rows tok_off[b] .. tok_off[b] + n_tok[b] - 1 of X
 * and its patch tokens rows tok_off[b] - b .. tok_off[b] - b + n_tok[b] - 2 of tok (n_tok, tok_off: int32 [B] on the device; tok_off[b] =
 * off_b / P + b for the sample offset off_b of record b).  N = the widest record's token count (n_tok[b] <= N).  The packed patch gather is
 * ecgvit_patch_gather with B = 1 over the (C, S) concatenation: patch row off_b / P + j of it is patch j of record b.
 * X[tok_off[b]] = cls + pos[0];  X[tok_off[b] + t] = tok[tok_off[b] - b - 1 + t] + pos[t];  embedding dropout by packed element index. */
int ecgvit_embed_finish_ragged(const void *tok, const float *cls, const float *pos, void *X, const int32_t *n_tok, const int32_t *tok_off,
                               int B, int N, int d, float dropout_p, uint64_t seed, int dtype, void *stream);
/* its backward: dtok of every patch token; dpos[t] = sum over the records with n_tok[b] > t of dX[tok_off[b] + t] for t < N (a fixed-order
 * gather per position: bit-reproducible); dcls = dpos[0] (f32 grads, overwritten; rows >= N of dpos are not touched) */
int ecgvit_embed_bwd_ragged(const void *dX, void *dtok, float *dcls, float *dpos, const int32_t *n_tok, const int32_t *tok_off, int B, int N,
                            int d, float dropout_p, uint64_t seed, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm (eps 1e-5, biased variance, affine).  replaces: vit_pytorch PreNorm.norm / mlp_head[0].
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_ROW_MAX_D 2048 /* d of the LayerNorm entry points and of ecgvit_pool_records (a multiple of 8): a row is held in one wave's registers */
int ecgvit_layernorm_fwd(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd,
                         int64_t rows, int d, float eps, int dtype, void *stream);
/* fp8 operand path: the same forward (bf16, d in 64 * {4, 8, 12, 16, 24, 32}) that also writes y8 = saturate(y / *q8_scale) in e4m3 and
 * accumulates *q8_amax = max(*q8_amax, max |y|): the 8-bit operand of the next Linear's product, without a quantise pass over y.
 * y may be NULL (ABI 5): only y8 / mean / rstd are written -- for a step in which every consumer of y reads the 8-bit copy.
 * mean, rstd and y meet the accuracy of ecgvit_layernorm_fwd but need not have its bits: the emitting kernel is an instantiation of its own whose
 * multiply-adds the compiler fuses differently, so rstd, and with it a few y per million, may differ in the last place (tests/test_gpu_layernorm.py) */
int ecgvit_layernorm_fwd_q8(const void *x, const float *gamma, const float *beta, void *y, float *mean, float *rstd,
                            int64_t rows, int d, float eps, void *y8, const float *q8_scale, float *q8_amax, void *stream);
/* dx = (dres ? dres : 0) + LN'(dy) ; dgamma/dbeta are OVERWRITTEN with the full reduction over rows.
 * `partial` is caller workspace of ecgvit_layernorm_bwd_workspace(rows, d) bytes. */
int64_t ecgvit_layernorm_bwd_workspace(int64_t rows, int d);
int ecgvit_layernorm_bwd(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd,
                         const void *dres, void *dx, float *dgamma, float *dbeta, void *partial,
                         int64_t rows, int d, int dtype, void *stream);

/* Same, plus what the next backward stage wants from dx while it is still in registers: dxm = dx * dropout_mask(seed, i)
 * (only written when dropout_p > 0) and dcolsum[c] = sum_rows (dropout_p > 0 ? dxm : dx) -- the gradient of the bias of the
 * `dropout(Linear + bias) + residual` site that produced x. */
int ecgvit_layernorm_bwd_fused(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd,
                               const void *dres, void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d,
                               void *dxm, float *dcolsum, float dropout_p, uint64_t seed, int dtype, void *stream);

/* Same, with the dropout bits of row r * mask_row_pitch for row r (a compact launch over one row per record; 1 == ecgvit_layernorm_bwd_fused) */
int ecgvit_layernorm_bwd_fused_rowpitch(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd,
                                        const void *dres, void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d,
                                        void *dxm, float *dcolsum, float dropout_p, uint64_t seed, int mask_row_pitch, int dtype, void *stream);

/* fp8 operand path: the same fused backward (bf16, d in 64 * {4, 8, 12, 16, 24, 32}) that also writes g8 = saturate(v / *q8_scale) in e5m2 for
 * v = the gradient the next stage consumes (dxm when dropout_p > 0, else dx; as stored) and accumulates *q8_amax = max(*q8_amax, max |v|):
 * the 8-bit A operand of that stage's input-gradient product, without a quantise pass over the gradient.
 * dxm may be NULL even with dropout_p > 0 (ABI 5): the masked gradient is then written as g8 only (dcolsum and g8 are unchanged) */
int ecgvit_layernorm_bwd_fused_q8(const void *dy, const void *x, const float *gamma, const float *mean, const float *rstd,
                                  const void *dres, void *dx, float *dgamma, float *dbeta, void *partial, int64_t rows, int d,
                                  void *dxm, float *dcolsum, float dropout_p, uint64_t seed, void *g8, const float *q8_scale,
                                  float *q8_amax, void *stream);

/* out[i] = in[i] * keep(seed, i) / (1-p): re-applies an epilogue dropout mask (element index = m*N+n, contiguous [M,N])
 * to the incoming gradient of a `dropout(acc + bias) + residual` site.  in == out allowed. */
int ecgvit_dropout_apply(const void *in, void *out, int64_t count, float dropout_p, uint64_t seed, int dtype, void *stream);
/* the same over a contiguous [rows, cols] slab whose row r takes the mask of row r * mask_row_pitch of a [*, cols] tensor (cols % 8 == 0) */
int ecgvit_dropout_apply_rows(const void *in, void *out, int64_t rows, int cols, int mask_row_pitch, float dropout_p, uint64_t seed, int dtype,
                              void *stream);

/* out[n] = sum_m in[m,n]  (bias gradients).  `partial`: ecgvit_colsum_workspace(M,N) bytes. */
int64_t ecgvit_colsum_workspace(int64_t M, int N);
int ecgvit_colsum(const void *in, int64_t ld, float *out, void *partial, int64_t M, int N, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-head self-attention core, fused (bf16 path).  replaces vit_pytorch Attention.forward between
 * to_qkv and to_out: split heads, dots = q k^T * dh^-0.5, softmax, (dropout), attn v, merge heads.
 * qkv: [B*N, 3*h*dh] (columns [q | k | v], head-major inside each) ; out: [B*N, h*dh] ; lse: [B,h,N] f32.
 * bf16 path requires dh == 64 or dh == 128 and N <= ECGVIT_ATTN_MAX_N; every other dh returns ECGVIT_EINVAL.  dh == 64: online softmax over 32-key tiles;
 * the backward takes N > 256 as one launch per 256-key window, each window after the first adding its dQ to the bf16 dQ already in dqkv.
 * dh == 128: online softmax over 64-key windows; the backward is two launches (dK / dV per 128-key block, then dQ with P recomputed), no
 * accumulation across launches.  Same layouts, LSE convention and dropout bits for both head dims.  Dropout hash index (bh N + q) ceil(N/4) + key/4 is uint32 and
 * wraps for B h N ceil(N/4) >= 2^32 (e.g. B h = 8192 at N > ~1 450): deterministic, a mask repeats there.
 * Probability dropout of the fused kernels: one 8-bit hash per 4 consecutive keys, so the probability APPLIED is
 * round(256 p) / 256 (p = 0.1 -> 26/256 = 0.1016), kept values rescaled by the exact 256 / (256 - round(256 p)); 0 < p < 1/512 cannot be
 * represented and is rejected (ECGVIT_EINVAL) rather than silently rounded to no dropout.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_ATTN_MAX_N 2048 /* tokens per record of the fused bf16 attention: every fused entry point (forward, backward, CLS-row, varlen, ragged,
                                  rollout) returns ECGVIT_EINVAL above it */
int ecgvit_attention_fwd(const void *qkv, void *out, float *lse, int B, int N, int h, int dh, float scale,
                         float dropout_p, uint64_t seed, int dtype, void *stream);
/* fp8 operand path (dh == 64 only: ECGVIT_EINVAL for dh == 128, the caller quantises `out` itself): the same forward that also writes out8 = saturate(out as stored / *q8_scale) in e4m3 (same [B*N, h*dh] layout, one byte
 * per element, 16-byte aligned) and accumulates *q8_amax = max(*q8_amax, max |out|): the 8-bit operand of the out-projection's product, without a quantise pass */
int ecgvit_attention_fwd_q8(const void *qkv, void *out, float *lse, int B, int N, int h, int dh, float scale, float dropout_p,
                            uint64_t seed, void *out8, const float *q8_scale, float *q8_amax, void *stream);
int ecgvit_attention_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv,
                         int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, int dtype,
                         void *stream);
/* fp8 operand path (dh == 64 and 128 < N <= 512 only: ECGVIT_EINVAL otherwise -- also for 512 < N <= 2048 -- the caller then quantises dqkv itself): the same backward that also writes
 * dqkv8 = saturate(dqkv as stored / *q8_scale) in e5m2 (same [B*N, 3*h*dh] layout, one byte per element) and accumulates
 * *q8_amax = max(*q8_amax, max |dqkv|): the 8-bit operand of the QKV projection's two backward products, without a quantise pass */
int ecgvit_attention_bwd_q8(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv,
                            int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *dqkv8,
                            const float *q8_scale, float *q8_amax, void *stream);
/* CLS-row attention (the pruned last block of the supervised step: the classifier reads row 0 of each record only).  Query row 0 of every
 * (record, head) against all N keys of `qkv` (layout as above): out_cls [B, h*dh] compact = row 0 of ecgvit_attention_fwd's out,
 * lse_cls [B, h] = its log-sum-exp, the same attention-dropout bits (bf16, dh == 64 or 128, N <= 2048). */
int ecgvit_attention_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, int B, int N, int h, int dh, float scale, float dropout_p,
                             uint64_t seed, int dtype, void *stream);
/* its backward for an upstream gradient dout_cls [B, h*dh] on row 0 only: writes the K and V columns of dqkv for EVERY row (what
 * ecgvit_attention_bwd writes there for a dout that is zero outside row 0) and dq_cls [B, h*dh] = the Q gradient of row 0; the Q columns of
 * dqkv are not touched. */
int ecgvit_attention_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv, void *dq_cls,
                             int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, int dtype, void *stream);
/* export of the fused path's post-softmax probabilities (next row f3; what vit_pytorch's Recorder hooks, reference ecg_vit.py:176-180):
 * probs[B,h,N,N] f32 = exp(scale * q k^T - lse), from the qkv / lse a fused forward left behind. bf16 path only (the f32 path
 * materialises the scores anyway); visualisation-time, not tuned. B*h <= 65535. */
int ecgvit_attention_probs(const void *qkv, const float *lse, float *probs, int B, int N, int h, int dh, float scale, int dtype,
                           void *stream);
/* Variable-length records (attention_varlen.hip): the same fused attention for a batch whose records hold n_tok[b] valid tokens, n_tok an int32
 * [B] DEVICE array with 1 <= n_tok[b] <= N; the row stride per record stays N.  Keys >= n_tok[b] take no part, rows >= n_tok[b] of out and
 * of all three parts of dqkv are written as exact zeros (their lse: 0), and the dropout bits are those of the uniform kernels for the batch N
 * (so a record's mask differs from the one it would draw alone at its own length).  bf16, dh == 64 or 128, N <= 2048.  The CLS forms are
 * ecgvit_attention_cls_fwd / _cls_bwd over the n_tok[b] keys; the backward writes zeros into the K / V rows >= n_tok[b]. */
int ecgvit_attention_varlen_fwd(const void *qkv, void *out, float *lse, const int32_t *n_tok, int B, int N, int h, int dh, float scale,
                                float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_varlen_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, const int32_t *n_tok,
                                int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_varlen_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, const int32_t *n_tok, int B, int N, int h, int dh,
                                    float scale, float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_varlen_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv,
                                    void *dq_cls, const int32_t *n_tok, int B, int N, int h, int dh, float scale, float dropout_p,
                                    uint64_t seed, void *stream);
/* Ragged batch (attention_varlen.hip, the same kernel bodies): record b's n_tok[b] tokens are the rows tok_off[b] .. tok_off[b] + n_tok[b] - 1
 * of qkv / out / dqkv (packed, no padded rows: nothing else is read or written).  N = the widest record's token count: it sets the lse layout
 * ((b h + head) N + q, rows >= n_tok[b] not written) and the dropout bits, which are those of ecgvit_attention_varlen_* at that N. */
int ecgvit_attention_ragged_fwd(const void *qkv, void *out, float *lse, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h,
                                int dh, float scale, float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_ragged_bwd(const void *qkv, const void *out, const void *dout, const float *lse, void *dqkv, const int32_t *n_tok,
                                const int32_t *tok_off, int B, int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_ragged_cls_fwd(const void *qkv, void *out_cls, float *lse_cls, const int32_t *n_tok, const int32_t *tok_off, int B,
                                    int N, int h, int dh, float scale, float dropout_p, uint64_t seed, void *stream);
int ecgvit_attention_ragged_cls_bwd(const void *qkv, const void *out_cls, const void *dout_cls, const float *lse_cls, void *dqkv,
                                    void *dq_cls, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int h, int dh, float scale,
                                    float dropout_p, uint64_t seed, void *stream);
/* f32 parity path pieces (scores materialised; the GEMMs are ecgvit_gemm batched calls):
 * in-place row softmax of S[rows, ld] over the first N columns; optional export is the buffer itself. */
int ecgvit_softmax_rows(float *S, int64_t rows, int N, int64_t ld, void *stream);
/* the f32 path's softmax for variable-length records: S[(b h + head) N + q][ld] over the first n_tok[b] columns (n_tok: int32 [B] on the
 * device); columns >= n_tok[b] and whole rows q >= n_tok[b] become 0, so ecgvit_softmax_bwd_rows gives dS = 0 there. */
int ecgvit_softmax_rows_varlen(float *S, const int32_t *n_tok, int B, int h, int N, int64_t ld, void *stream);
/* dS = P * (dP - rowsum(P*dP)) * scale, written over dP */
int ecgvit_softmax_bwd_rows(const float *P, float *dP, int64_t rows, int N, int64_t ld, float scale, void *stream);

/* ------------------------------------------------------------------------------------------------
 * classification head + loss.  replaces: x[:,0] -> mlp_head (LayerNorm, Linear(d,K)) and
 * nn.BCEWithLogitsLoss (reference ecg_vit.py:118, :144-148).
 * ------------------------------------------------------------------------------------------------ */
/* logits[b,c] = LN(X[b*N+0]) . W[c,:] + bias[c] ; saves xhat [B,d] f32 and rstd [B] for backward */
int ecgvit_head_fwd(const void *X, int N, const float *gamma, const float *beta, const float *W, const float *bias,
                    float *logits, float *xhat, float *rstd, int B, int d, int K, float eps, int dtype, void *stream);
/* elementwise l = w * (max(z,0) - z*y + log1p(exp(-|z|))) ; loss_elem [B*K] always written;
 * loss_mean (1 f32) = mean(l) if non-NULL.  weight may be NULL.  Deterministic single-pass reduction. */
int ecgvit_bce_fwd(const float *logits, const float *labels, const float *weight, float *loss_elem, float *loss_mean,
                   int64_t count, void *stream);
/* dlogits = upstream * w * (sigmoid(z) - y) ; upstream = *gscalar * gscale (gelem NULL) or gelem[i] * gscale */
int ecgvit_bce_bwd(const float *logits, const float *labels, const float *weight, const float *gscalar,
                   const float *gelem, float gscale, float *dlogits, int64_t count, void *stream);
/* backward of head_fwd: dW,dbias,dgamma,dbeta overwritten; dX [B*N, d] is ZERO-FILLED then CLS rows written */
int ecgvit_head_bwd(const float *dlogits, const float *xhat, const float *rstd, const float *gamma, const float *beta,
                    const float *W, float *dW, float *dbias, float *dgamma, float *dbeta, void *dX, int N, int B, int d,
                    int K, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------------
 * optimiser: global-norm clip + AdamW/Adam over FLAT f32 buffers.  replaces train.py:281-282
 * (nn.utils.clip_grad_norm_(max_norm=1.0, error_if_nonfinite=True) + torch.optim.AdamW.step).
 * ------------------------------------------------------------------------------------------------ */
int64_t ecgvit_sumsq_workspace(int64_t count);
/* out[0] = sum(g^2) (f32, deterministic two-stage) ; `partial` = ecgvit_sumsq_workspace(count) bytes */
int ecgvit_sumsq(const float *g, int64_t count, float *out, void *partial, void *stream);
/* norm = |grad_scale| * sqrt(sumsq[0]) ; coef = min(1, max_norm / (norm + 1e-6)) (coef = 1 if max_norm <= 0);
 * g' = g * grad_scale * coef ; AdamW: p *= 1 - lr*wd ; Adam: g' += wd * p ; m,v update ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 * norm_out[0] = norm (pre-clip, of grad_scale-scaled grads), norm_out[1] = 1.0 if norm is finite else 0.0;
 * when the norm is non-finite NOTHING is updated (caller raises, as error_if_nonfinite=True does).
 * p_lowp: optional bf16 shadow copy of p, refreshed in the same pass. */
int ecgvit_adamw_step(float *p, const float *g, float *m, float *v, void *p_lowp, int64_t count,
                      const float *sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2,
                      float eps, float weight_decay, int step, int decoupled, float *norm_out, void *stream);
/* The same two passes over a SPAN TABLE of the flat buffers (frozen parameters: only trainable ones are counted and updated).
 * spans (DEVICE, int64 [nspan][3]) = {element offset, count, step offset}; total = the sum of the counts (sizes the grid).
 * ecgvit_sumsq_spans: out[0] = sum of g^2 over the spans (f32, deterministic two-stage; `partial` = ecgvit_sumsq_spans_workspace bytes).
 * ecgvit_adamw_step_spans: ecgvit_adamw_step restricted to the spans; span s takes its bias corrections at step + spans[s][2] (its own
 * optimiser step count, as torch keeps state['step'] per parameter); lr is the caller's, from the global step.  Elements outside the
 * spans are neither read nor written.  Non-finite norm: nothing is updated, norm_out[1] = 0. */
int64_t ecgvit_sumsq_spans_workspace(int nspan);
int ecgvit_sumsq_spans(const float *g, const int64_t *spans, int nspan, int64_t total, float *out, void *partial, void *stream);
int ecgvit_adamw_step_spans(float *p, const float *g, float *m, float *v, void *p_lowp, const int64_t *spans, int nspan, int64_t total,
                            const float *sumsq, float grad_scale, float max_norm, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int step, int decoupled, float *norm_out, void *stream);
/* Gradient accumulation over micro-batches (HipTrainStep.step(..., micro_batch_size=)); replaces what the reference left as
 * `# TODO: gradient accumulation not supported` (models/train.py:431).  Each backward pass overwrites g (the flat gradient buffer); acc is
 * a second flat f32 buffer of the same layout.  Over the spans (the span table above; step offsets unused):
 *   ECGVIT_ACC_INIT  acc = scale * g          (after the first micro-batch)
 *   ECGVIT_ACC_ADD   acc += scale * g         (after each middle micro-batch)
 *   ECGVIT_ACC_FOLD  g = scale * g + acc      (the last micro-batch: g then holds the whole batch's gradient for the norm, the exchange and AdamW)
 * scale = 1 for gradients (exact); total = the sum of the counts (sizes the grid).  acc and g 16-B aligned; span offsets should be multiples
 * of 4 elements (16-B accesses; others take the element path).  Elements outside the spans are neither read nor written. */
#define ECGVIT_ACC_INIT 0
#define ECGVIT_ACC_ADD 1
#define ECGVIT_ACC_FOLD 2
int ecgvit_grad_accumulate(float *acc, float *g, const int64_t *spans, int nspan, int64_t total, int mode, float scale, void *stream);
/* g *= min(1, max_norm/(norm+1e-6)) in place (torch-optimizer interop path); norm_out as above */
int ecgvit_clip_scale(float *g, int64_t count, const float *sumsq, float max_norm, float *norm_out, void *stream);
int ecgvit_cast_f32_to_bf16(const float *src, void *dst, int64_t count, void *stream);
int ecgvit_cast_bf16_to_f32(const void *src, float *dst, int64_t count, void *stream);
/* Transposed bf16 shadows of the Linear weights: with W^T at hand the input-gradient product dX = dY . W (nn.Linear backward) runs
 * on the forward (A . B^T) kernel.  src / dst: flat bf16 buffers with identical layouts; table (DEVICE, int64 [nmat][4]) =
 * {element offset, rows, cols, index of the matrix's first 64x64 tile}; dst + offset receives the cols x rows transpose.
 * ntiles = total number of 64x64 tiles over all matrices. */
int ecgvit_transpose_bf16_batched(const void *src, void *dst, const int64_t *table, int nmat, int64_t ntiles, void *stream);

/* ------------------------------------------------------------------------------------------------
 * masked pre-train objective (build's own definition; absent from the reference)
 * ------------------------------------------------------------------------------------------------ */
/* tok[b*n + idx[b,k]] = mask_token for k < m (idx int32, distinct per record) then X = tok + pos[1..n] (no CLS row).
 * flag_ws: caller scratch of B*n bytes. */
int ecgvit_mask_embed_finish(const void *tok, const float *mask_token, const float *pos, const int32_t *idx, void *X,
                             void *flag_ws, int B, int n, int m, int d, int dtype, void *stream);
/* backward: dtok = dX on un-masked rows (0 elsewhere), dmasked = dX on masked rows (0 elsewhere; its column sum is the
 * mask-token gradient), dpos[1+p] = sum_b dX[b*n+p], dpos[0] = 0.  flag_ws as written by ecgvit_mask_embed_finish. */
int ecgvit_mask_embed_bwd(const void *dX, const void *flag_ws, void *dtok, void *dmasked, float *dpos, int B, int n, int d,
                          int dtype, void *stream);
/* The same pair for records of unequal length.  Record b holds n_tok[b] >= 1 patches in the rows tok_off[b] .. tok_off[b] + n_tok[b] - 1
 * of tok / X / dX / dtok / dmasked (n_tok, tok_off: int32 [B] on the device); N = the largest n_tok; M = all rows.  Two row layouts:
 *   packed  n_pad == 0: tok_off = the exclusive prefix sum of n_tok, M = sum n_tok; no other row exists
 *   padded  n_pad >= N: tok_off[b] = b * n_pad, M = B * n_pad; rows past n_tok[b] are never read and written as exact zeros (X, dtok, dmasked)
 * forward: X[row] = (masked ? mask_token : tok[row]) + pos[1 + j] for patch j of its record; row_idx (int32 [m_total], device) = the masked
 * rows of the pass (tok_off[b] + record-local index: distinct, in [0, M); others are ignored); flag_ws: caller scratch of M bytes.
 * backward: dtok / dmasked split by the flag; dpos[1 + j] = sum over the records with n_tok > j of their row j, rows 0 and those past the
 * widest record (up to 1 + n_pad in the padded layout, 1 + N packed) exact zeros; summed in a fixed order (bit-identical from launch to
 * launch).  order: int32 [B] on the device, the records by falling n_tok (ties by rising record index).  B <= 65535. */
int ecgvit_mask_embed_varlen_fwd(const void *tok, const float *mask_token, const float *pos, const int32_t *row_idx, void *X, void *flag_ws,
                                 const int32_t *n_tok, const int32_t *tok_off, int B, int N, int n_pad, int64_t M, int m_total, int d,
                                 int dtype, void *stream);
int ecgvit_mask_embed_varlen_bwd(const void *dX, const void *flag_ws, void *dtok, void *dmasked, float *dpos, const int32_t *n_tok,
                                 const int32_t *tok_off, const int32_t *order, int B, int N, int n_pad, int d, int dtype, void *stream);
/* gather rows: out[b*m + k] = in[b*n + idx[b,k]] */
int ecgvit_gather_rows(const void *in, const int32_t *idx, void *out, int B, int n, int m, int64_t width, int64_t ld_in,
                       int64_t ld_out, int dtype, void *stream);
/* scatter-add rows (distinct idx per record => plain stores into a zero-filled buffer) */
int ecgvit_scatter_rows(const void *in, const int32_t *idx, void *out, int B, int n, int m, int64_t width,
                        int64_t ld_in, int64_t ld_out, int dtype, void *stream);
/* L1 reconstruction loss: loss[0] = mean |pred - target| ; dpred = upstream * sign(pred - target) / count.
 * partial: >= 1024 floats of scratch (per-block partial sums of the deterministic two-stage reduction). */
int ecgvit_l1_loss_fwd_bwd(const void *pred, const void *target, float *loss, void *dpred, const float *gscalar, float *partial,
                           int64_t rows, int width, int64_t ld, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------------
 * evaluation metrics (next row f1).  replaces: get_accuracy (ecg_transformer/util/train.py:12-56), called on every train
 * step (models/train.py:289) and after each eval pass (models/train.py:371) -- there a D2H copy of the logits + sklearn.
 * scores / labels: (B, K) f32 with row pitches ld_*; scores are probabilities, or logits when from_logits != 0 (then the f32
 * sigmoid the reference applies first, models/train.py:369, is evaluated in the kernel).  counts: uint64 [4 + 2K], overwritten:
 *   [0..3] tp, tn, fp, fn of (prob >= 0.5) over all B*K;  [4 + c] positives of class c;
 *   [4 + K + c] sum over (positive i, negative j) of 2*[p_i > p_j] + [p_i == p_j]  (AUROC_c = that / (2 P_c N_c)); 0 unless with_auc.
 * ------------------------------------------------------------------------------------------------ */
int ecgvit_eval_counts(const float *scores, int64_t ld_scores, const float *labels, int64_t ld_labels, int64_t B, int K, int from_logits,
                       int with_auc, uint64_t *counts, void *stream);

/* ------------------------------------------------------------------------------------------------
 * record pooling (EcgVit.encode): one f32 vector per record from its token rows.  Additive entry point: the ABI version stays 6.
 * x: token rows [*, d] (dtype bf16 / f32); record b holds n_tok[b] rows (N when n_tok is NULL; 1 <= n_tok[b] <= N) starting at row
 * tok_off[b] (b * N when tok_off is NULL) -- int32 device arrays, the convention of ecgvit_attention_ragged_* / ecgvit_embed_finish_ragged.
 * mode ECGVIT_POOL_CLS: the record's row 0 (the CLS row);  mode ECGVIT_POOL_MEAN: the mean over its n_tok[b] rows, CLS row included (vit_pytorch pool='mean').
 * Rows at or past n_tok[b] are never read.  gamma / beta non-NULL (both or neither): LayerNorm over d (biased variance, eps) of the pooled
 * f32 vector before the store (vit.mlp_head.0: what the classifier's Linear reads).  out: [B, d] f32, compact.
 * d a multiple of 8, at most ECGVIT_ROW_MAX_D.  f32 accumulation in an order fixed by the record's own row count: no atomics, bit-reproducible, and
 * independent of B, of the other records and of the row base (packed and padded rows pool to the same bits).
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_POOL_CLS 0  /* mode: the record's row 0 */
#define ECGVIT_POOL_MEAN 1 /* mode: the mean over the record's n_tok[b] rows */
int ecgvit_pool_records(const void *x, float *out, const int32_t *n_tok, const int32_t *tok_off, int B, int N, int d, int mode,
                        const float *gamma, const float *beta, float eps, int dtype, void *stream);

/* ------------------------------------------------------------------------------------------------
 * attention rollout for whole batches (EcgVit.attention_rollout_batch; next row f3).  replaces: the map EcgVitVisualizer derives per record
 * from vit_pytorch's Recorder (reference ecg_vit.py:164-194, :306-326), without an N x N matrix: with A_i = mean_head P_i of layer i and the
 * row sums of A_i + I taken as exactly 2 (softmax rows sum to 1), the reference's res[i][0, 1:] is
 *   c_i[k] = (A_i[0,k] + [k == 0]) / 2 ;  r_0 = c_0 ;  r_i[k] = (sum_q c_i[q] A_{i-1}[q,k] + c_i[k]) / 2 ;  map[i][k-1] = r_i[k] / max r.
 * Additive entry points: the ABI version stays 6.
 * qkv, lse, n_tok, tok_off, N, scale: exactly as ecgvit_attention_fwd / _varlen_fwd / _ragged_fwd take and leave them (lse natural-log units,
 * as ecgvit_attention_probs reads it).  n_tok == NULL: every record holds N tokens; tok_off != NULL: packed rows (lse at (b h + head) N + q).
 * Rows q >= n_tok[b] and keys k >= n_tok[b] are never read as data.  c, w, r: f32 [B, N]; entries at k >= n_tok[b] are written as 0.
 * dtype ECGVIT_BF16: P is rebuilt from qkv / lse (probs must be NULL): dh == 64 or 128, N <= 2048, all three row layouts; S tiles by bf16 MFMA
 * with f32 accumulation, exp, weighting and the sum over q in f32.  dtype ECGVIT_F32: P is read from the materialised probs [B,h,N,N] of the
 * f32 path (qkv, lse, tok_off must be NULL; any dh): uniform and n_tok batches.  Anything else: ECGVIT_EINVAL, nothing launched.
 * No atomics: heads and query tiles are added in a fixed order that is a function of the record's own n_tok[b] and of h alone, so a record's
 * rows of c and r are bit-identical in a padded, a n_tok and a packed batch, alone or among others (as ecgvit_pool_records).
 * ------------------------------------------------------------------------------------------------ */
/* bytes of `workspace` ecgvit_rollout_colsum needs: the per-head column sums [B, h, N] f32 that its second stage adds in head order */
int64_t ecgvit_rollout_workspace(int B, int N, int h);
/* c[b,k] = (mean_head P[b,head,0,k] + [k == 0]) / 2: the row-normalised CLS row of (A + I) */
int ecgvit_rollout_cls(const void *qkv, const float *lse, const float *probs, float *c, const int32_t *n_tok, const int32_t *tok_off, int B, int N,
                       int h, int dh, float scale, int dtype, void *stream);
/* r[b,k] = ((1/h) sum_head sum_{q < n_tok[b]} w[b,q] P[b,head,q,k] + w[b,k]) / 2: the row vector w times the row-normalised (A + I) of the layer
 * whose qkv / lse (probs) are passed.  w != r.  Two launches: per (record, head, key block), then over the heads. */
int ecgvit_rollout_colsum(const void *qkv, const float *lse, const float *probs, const float *w, float *r, void *workspace, const int32_t *n_tok,
                          const int32_t *tok_off, int B, int N, int h, int dh, float scale, int dtype, void *stream);
/* maps: f32 [B, layers, N - 1], layer i of record b = r_i[1:] with zeros past n_tok[b] - 1.  Divides record b's rows by the maximum over its own
 * layers x (n_tok[b] - 1) entries (IEEE division: that maximum becomes exactly 1.0); entries past n_tok[b] - 1 are not touched, a record of one
 * token (an empty map) is left as it is. */
int ecgvit_rollout_finish(float *maps, const int32_t *n_tok, int B, int layers, int N, void *stream);

/* ------------------------------------------------------------------------------------------------
 * per-lead statistics of a record store (transform.fit_dynamic_normalize; next row f2).  replaces: the np.nanmean / nanstd / nanmin / nanmax /
 * nanpercentile sweeps DynamicNormalize makes over an (n, 12, L) host array (reference preprocess/transform.py:38-137, fitted at
 * util/config.py:296-308).  Additive entry points: the ABI version stays 6.
 * Records are addressed as ecgvit_patch_gather_transform_varlen addresses them: lead c of record r (r < R) = raw_len[r] f32 samples at
 * x + src_off[r] + c * lead_stride (src_off int64 [R], raw_len int32 [R], device arrays; raw_len[r] <= 0 skips the record).  A rectangular
 * (n, C, L) store, a ragged (C, S_total) one and any subset of either are tables over the same buffer; a record's first sample may sit at any
 * 4-byte address.  NaN samples are counted and otherwise left out, as the nan-functions leave them out; +-0, denormals and +-inf are ordinary
 * values.  Every entry point ADDS to state the caller owns and zeroes: a store larger than one launch is a sequence of launches per pass.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_FIT_TARGETS 16 /* order statistics per lead of one select: the second extent of sel and hist */
#define ECGVIT_FIT_BINS 256   /* bins per radix pass (8-bit digits): the third extent of hist */
/* bytes of `workspace` ecgvit_fit_moments needs for R records (the per-workgroup partials its second stage adds in a fixed order) */
int64_t ecgvit_fit_workspace(int R, int C);
/* state: per lead 32 bytes { uint64 count of non-NaN samples, uint64 count of NaN samples, double sum, double sum of squared deviations }.
 * mean == NULL: the first three are added to; mean != NULL (double [C], device): sum (x - mean[c])^2 is added to the fourth alone (np.nanstd is
 * two-pass, ddof 0).  f64 throughout, two stages in a fixed order, no floating-point atomics: the same launches give the same bits. */
int ecgvit_fit_moments(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, const double *mean,
                       void *workspace, void *state, void *stream);
/* Exact order statistics by radix select on the monotone uint32 key of the f32 bit pattern (k = bits ^ (bits < 0 ? ~0 : 0x80000000): -0.0 sorts
 * directly below +0.0), 8 bits per pass, passes 0..3.  sel: uint64 [C][ECGVIT_FIT_TARGETS][4] per (lead, target) { rank, key prefix, slot, count of the chosen
 * bin }; the caller writes the rank of each of its ntarget <= ECGVIT_FIT_TARGETS targets (0-based among the lead's non-NaN samples) and zeroes the rest.
 * hist: uint64 [C][ECGVIT_FIT_TARGETS][ECGVIT_FIT_BINS], zeroed by the caller before each pass.  Pass p:
 *   ecgvit_fit_histogram (once per launch of the store) counts digit p of every non-NaN sample whose key starts with a target's decided prefix
 *     (pass 0: every sample, slot 0); targets that share a prefix share a slot.  Integer atomics only: exact, independent of order;
 *   ecgvit_fit_select then finds, per target, the bin holding its rank, appends it to the prefix and leaves the rank within the bin -- on the
 *     device, so the passes queue without a host round trip.
 * After pass 3 the prefix is the key of the exact order statistic (bits = key & 0x80000000 ? key ^ 0x80000000 : ~key); a count of 0 there
 * means the rank was not below the lead's count. */
int ecgvit_fit_histogram(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, const uint64_t *sel,
                         int ntarget, int pass, uint64_t *hist, void *stream);
int ecgvit_fit_select(const uint64_t *hist, uint64_t *sel, int C, int ntarget, int pass, void *stream);

/* ------------------------------------------------------------------------------------------------
 * segment tokenizer (tokenizer.EcgTokenizer; the reference's symbolisation branch, models/ecg_tokenizer.py: EcgPadder :88-137, encode :222-258,
 * decode :346-350, the k-means fit :352-490 through sklearn).  Additive entry points: the ABI version stays 6.
 * The store is addressed as ecgvit_fit_moments addresses it (x, src_off, lead_stride, raw_len; a record starts at any 4-byte address).  Lead c of
 * record r is cut into raw_len[r] / k + 1 segments of k samples (k in {8, 16, 32}), padded INSIDE the segment load as EcgPadder pads:
 * n_pad = k - raw_len % k samples (a whole extra segment when k divides the length), pad == 0: zeros, pad == 1 ('shift'): position l + j holds
 * sample l - n_pad + j (the caller guarantees l >= n_pad; the kernels clamp the index to the run, so nothing outside a run is ever read).
 * The segments of one lead over the R records, in record order, are positions 0 .. n_seg - 1: seg_cum (int64 [R + 1], device, seg_cum[0] = 0,
 * seg_cum[r + 1] - seg_cum[r] = raw_len[r] / k + 1, seg_cum[R] = n_seg) maps a position to its record.  Segment s of (r, c) has its id, mean and
 * distance at element dst_off[r] + c * dst_stride + s of ids / means / dist (dst_off int64 [R], device): (n, C, T) outputs of a rectangle and
 * the (C, T_total) outputs of a ragged store are tables again.
 * Per segment: mean = (((x0 + x1) + x2) + ... ) * (1 / k) in f32, in that order whatever the layout or the batch; the segment minus its mean
 * is what is clustered.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_TOK_MAX_CLUSTERS 65536  /* rows of a centre table (V) */
#define ECGVIT_TOK_MAX_LOCAL_TRIALS 16 /* candidates per step of the k-means++ seeding (n_trials) */
#define ECGVIT_TOK_SEED_SPAN 1024      /* consecutive positions of one lead per workgroup of the seeding's sweep: sizes ecgvit_tok_seed_workspace */
#define ECGVIT_TOK_DBSCAN_TILE 256     /* segments per LDS tile of a DBSCAN sweep's column side: what ecgvit_tok_dbscan_tile() returns */
/* ids[.] = argmin_j |s - c_j|^2 over the V rows of centers (f32 [V][k], 1 <= V <= ECGVIT_TOK_MAX_CLUSTERS), means[.] = the segment's mean, dist[.] (may be NULL)
 * = sum_e (s_e - c_e)^2 for the chosen centre, recomputed directly.  The argmin is taken on score_j = |c_j|^2 - 2 s . c_j, an f32 fma chain
 * in sample order on the matrix pipe (v_mfma_f32_32x32x2_f32, exact f32) that starts from |c_j|^2; equal scores go to the smaller index.
 * prev_ids != NULL (may be ids itself): *changed (uint64, device; zeroed by this call) receives the number of segments whose id differs from
 * prev_ids; prev_ids and changed come together or not at all.  Integer atomics only. */
int ecgvit_tok_assign(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, const float *centers, int V,
                      const int32_t *prev_ids, int32_t *ids, float *means, float *dist, uint64_t *changed, void *stream);
/* bytes of `workspace` ecgvit_tok_update needs (int64 sums [V][k], uint64 counts [V], the absolute maximum); 0 for an unsupported (V, k) */
int64_t ecgvit_tok_workspace(int V, int k);
/* One Lloyd update: centers[j] = the mean of the mean-removed segments with ids[.] == j, lens[j] (int64 [V]) = their number; a centre that
 * receives no segment keeps its value and reports 0; ids outside [0, V) are left out.  Three launches after zeroing the workspace: the absolute
 * maximum A of the mean-removed samples (keep_amax == 1: that sweep is skipped and the maximum the previous call left in this workspace is used
 * again -- it depends on the store and the padding alone, not on ids, so one sweep serves every update of a fit over one store; 0 or 1) (integer atomic max on the bits); per sample q = rint(v * 2^(31 - E)) with 2^(E - 1) <= A < 2^E, added
 * to its centre's int64 sum by 64-bit integer atomics (addition of integers has no order: the same launches give the same bits); the division
 * in f64.  |q| <= 2^31, so a sum holds 2^32 - 1 segments without overflow: C * n_seg >= 2^32 is refused with ECGVIT_EINVAL.  The rounding
 * of q is at most A * 2^-31 per sample, and so per centre element (an absolute error: a centre element near zero has no relative bound; the
 * tests hold max_e |c32 - c64| to 1e-6 max_e |c64| per centre). */
int ecgvit_tok_update(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, const int32_t *ids,
                      float *centers, int V, int64_t *lens, void *workspace, int keep_amax, void *stream);
/* k-means++ seeding: sklearn.cluster.kmeans_plusplus (the greedy `_kmeans_plusplus`) over the mean-removed segments of the store, with the
 * generator's draws handed in and every sum an integer.  It is sklearn's algorithm, not its random stream.
 *   segment index   g = c * n_seg + p: lead c, position p among that lead's segments in record order -- the same for a rectangle, a ragged
 *                   store, an idxs subset and its compact copy.
 *   distance        d2 = sum_e (s_e - c_e)^2 in f32, UNFUSED: every difference, product and addition rounds on its own, in sample order from
 *                   the first product; s as every tokenizer kernel loads it (the f32 mean rule above).  closest(g) = the smallest d2 to the
 *                   centres chosen so far, taken with a strict < from +inf (a NaN distance changes nothing).
 *   weight          q = rint(d2 * 2^F) as uint64, computed in f64 where the product is exact (ties to even: a distance of half a unit or less
 *                   weighs 0 and cannot be drawn); F = 63 - H - (2 E + 2 + log2 k) with 2^(E - 1) <= A < 2^E for the absolute maximum A of the
 *                   mean-removed samples (the sweep of ecgvit_tok_update, its exponent rule) and H = bit_length(C * n_seg).  d2 <= k (2 A)^2
 *                   < 2^(2 E + 2 + log2 k), so q <= 2^(63 - H) and every potential (the sum of q over all segments) is below 2^63: no overflow
 *                   check exists.  C * n_seg >= 2^32 is refused.  The unit 2^-F is 2^-(61 - H) of k (2 A)^2: at 2^28 segments and k = 8,
 *                   2^-30 of 32 A^2.  A segment whose distance is not finite (it holds a non-finite sample) weighs 0.
 *   step 0          centre 0 is segment `first` (0 <= first < C * n_seg).
 *   step c >= 1     with pot = the potential under centres 0 .. c - 1, trial t (0 <= t < n_trials, 1 .. ECGVIT_TOK_MAX_LOCAL_TRIALS) draws target =
 *                   (u53[(c - 1) * n_trials + t] * pot) >> 53 from the 117-bit product (u53: device uint64, each below 2^53 -- floor(u 2^53) of
 *                   a uniform u in [0, 1)); its candidate is the smallest g whose inclusive running sum of q exceeds the target (a segment of
 *                   weight 0 is never drawn), and g = 0 when pot == 0 (every segment coincides with a chosen centre: what sklearn's searchsorted
 *                   returns there).  The candidate that leaves the smallest potential becomes centre c; equal potentials go to the smaller t.
 * centers (f32 [V][k]) receives the chosen segments (mean removed, bit for bit what the kernels load), indices (int64 [V]) their g; trace (NULL,
 * or uint64 [V - 1][n_trials][2]) every trial's candidate g and the potential it leaves.  V <= C * n_seg.  u53 may be NULL when V == 1.
 * keep_amax == 1: the sweep for A is skipped and the maximum a previous seeding left at the start of this workspace is used again (the first
 * 16 bytes of the workspace hold what the last 16 bytes of ecgvit_tok_update's hold: the bits of A, then zeros).
 * 2 V launches after that sweep, all on `stream`: no host read, allocation or synchronisation.  Per centre a sweep reads the store once, updates
 * closest (4 bytes read and written per segment) and leaves one uint64 per (trial, workgroup of ECGVIT_TOK_SEED_SPAN consecutive positions of one lead); a
 * one-workgroup pick sums them, takes the argmin and finds the next candidates by a scan of the winner's sums and of one span.  No atomics:
 * integer addition has no order, so the same arguments give the same bits, and a record gives the same weights in every store form. */
int64_t ecgvit_tok_seed_workspace(int C, int64_t n_seg, int V, int k, int n_trials);   /* bytes; 0 when unsupported */
int ecgvit_tok_seed(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                    const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, int V, int n_trials, int64_t first,
                    const uint64_t *u53, float *centers, int64_t *indices, uint64_t *trace, void *workspace, int keep_amax, void *stream);
/* out (the store's own layout: lead c of record r at out + src_off[r] + c * lead_stride) = centers[ids] + means, truncated to raw_len[r]
 * samples: the reference's decode plus the mean it adds back (:292).  A segment whose id lies outside [0, V) is written as NaN. */
int ecgvit_tok_decode(float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                      const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, const int32_t *ids, const float *means,
                      const float *centers, int V, void *stream);
/* DBSCAN (sklearn.cluster.DBSCAN, the reference's `dbscan` clustering) over the same mean-removed segments (dbscan.hip).  Additive entry
 * points: the ABI version stays 6.  It is sklearn's algorithm, not its arithmetic: sklearn compares distances in f64.
 *   order           the reference's flat order sigs.reshape(-1, k): record first (in the selection's order), then lead, then segment.  Segment s
 *                   of lead c of record r is q = C * seg_cum[r] + c * n_r + s with n_r = seg_cum[r + 1] - seg_cum[r] -- the same rule for a
 *                   rectangle, a ragged store and an idxs subset, so a record set gives the same labels in every store form.  n = C * n_seg
 *                   < 2^31.
 *   neighbours      i and j are neighbours iff d2(x_i, x_j) <= eps2, d2 the unfused f32 chain of the seeding (sum_e (a_e - b_e)^2 in sample
 *                   order; every difference, product and addition rounds on its own) and eps2 = fl32(fl32(eps) * fl32(eps)), formed by the
 *                   caller.  The chain is bit-symmetric in its arguments, so the graph is undirected, and a segment is its own neighbour.  A
 *                   segment with a non-finite sample fails every comparison, its own too: it is nobody's neighbour and ends as noise.  The
 *                   relative rounding error of the chain is at most (k + 2) 2^-24: the result differs from an f64 evaluation only where a pair
 *                   lies that close to eps.
 *   core            a segment whose neighbour count, itself included, is at least min_samples (the caller's comparison on `count`).
 *   clusters        the connected components of the core segments under the neighbour relation, numbered 0, 1, ... by the smallest q among
 *                   their core members.
 *   border, noise   a non-core segment with a core neighbour takes the smallest label among its core neighbours, one with none is -1.  This is
 *                   sklearn's result: it grows clusters one at a time in index order of their first core point and never relabels a point.
 * ecgvit_tok_segments writes the dense table every later pass reads: segs (f32 [n][k], 16-byte aligned) = the mean-removed segments, bit for bit
 * what every tokenizer kernel loads, and means (f32 [n]), both in q order; dst (NULL, or int64 [n]) = where segment q has its id in the (n, C, T)
 * / (C, T_total) outputs of ecgvit_tok_assign (dst_off[r] + c * dst_stride + s).
 * The pair sweeps take rows [row0, row1) of a table per call (0 <= row0 < row1 <= rows), so that the caller bounds the pairs of one launch; a
 * workgroup holds ecgvit_tok_dbscan_rows(k) rows in registers and streams the other table through LDS in tiles of ecgvit_tok_dbscan_tile()
 * == ECGVIT_TOK_DBSCAN_TILE segments.  No floating-point atomics, and no atomics at all outside `link`.
 *   count   count[i] (int32 [n]) = the number of j in [0, n) with d2(segs_i, segs_j) <= eps2, for i in [row0, row1); one plain store per row.
 *   link    core: the core segments in ascending q (f32 [m][k]); parent: int32 [m], parent[x] = x before the first call.  Rows i in [row0,
 *           row1) meet the columns j < i; every edge joins the trees of i and j in a lock-free union-find: parent[x] <= x always, a find walks
 *           down with relaxed loads, a union hooks the larger root under the smaller with an integer atomic min and, where that shows the
 *           larger had been hooked meanwhile, goes on from the value it got back.  Every loop strictly descends indices and none waits for
 *           another workgroup.  After all rows the root of a tree is its component's smallest index: the result has no run-to-run variation.
 *   flatten root[i] (int32 [m]) = the root of core row i.  Ascending roots are ascending smallest q: their ranks are the labels.
 *   border  rows: the non-core segments (f32 [nrows][k]); label[i] (int32 [nrows]) = the smallest core_label[j] (int32 [m], >= 0) over the core
 *           rows j with d2 <= eps2, or -1, for i in [row0, row1).
 * k in {8, 16, 32}, 0 <= eps2 < inf; anything else is ECGVIT_EINVAL and launches nothing. */
int ecgvit_tok_segments(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, const int64_t *seg_cum,
                        const int64_t *dst_off, int64_t dst_stride, int R, int C, int64_t n_seg, int k, int pad, float *segs, float *means,
                        int64_t *dst, void *stream);
int ecgvit_tok_dbscan_tile(void);        /* segments per LDS tile of a sweep's column side */
int ecgvit_tok_dbscan_rows(int k);       /* rows per workgroup of a sweep; 0 for an unsupported k */
int ecgvit_tok_dbscan_count(const float *segs, int n, int k, float eps2, int row0, int row1, int32_t *count, void *stream);
int ecgvit_tok_dbscan_link(const float *core, int m, int k, float eps2, int row0, int row1, int32_t *parent, void *stream);
int ecgvit_tok_dbscan_flatten(const int32_t *parent, int m, int32_t *root, void *stream);
int ecgvit_tok_dbscan_border(const float *rows, int nrows, const float *core, const int32_t *core_label, int m, int k, float eps2, int row0, int row1,
                             int32_t *label, void *stream);

/* ------------------------------------------------------------------------------------------------
 * the Zheng et al. denoiser (denoise.py; the reference's preprocess/data_preprocessor.py:22-148 and its MATLAB twin): zero-phase low-pass, robust
 * LOESS baseline, noise estimate, non-local means.  Additive entry points: the ABI version stays 6.
 * The store is addressed as ecgvit_fit_moments addresses it (x, src_off, lead_stride, raw_len; raw_len[r] <= 0 skips a record; a record starts
 * at any 4-byte address).  max_len: the caller's upper bound of raw_len, at most ECGVIT_DENOISE_MAX_LEN (the non-local means and the robust LOESS keep a lead in
 * LDS; the _long / _tiled entry points at the end of this section take up to ECGVIT_DENOISE_MAX_LEN_TILED); a record longer than max_len is left untouched.  out: the store's own layout (lead c of record r at out + src_off[r] + c * lead_stride); out == x runs in
 * place, any other overlap is the caller's error.  Only the selected records' raw_len samples are written.  One workgroup per (record, lead);
 * every sum runs in an order that is a function of the record's own length and of the parameters alone, without floating-point atomics: a
 * record's output has the same bits in a rectangle, a ragged store or a subset, alone or in a batch.  NaN input is not supported.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_DENOISE_MAX_LEN 32768          /* max_len of the resident entry points: the non-local means keeps a lead in LDS */
#define ECGVIT_DENOISE_MAX_LEN_TILED 33554432 /* max_len of the _long / _tiled entry points: 1 << 25 samples, 24 hours at 360 Hz */
#define ECGVIT_DENOISE_MAX_TAPS 9             /* ntaps of ecgvit_filtfilt */
#define ECGVIT_DENOISE_MAX_POINTS 1024        /* samples per regression window of ecgvit_rloess (npoints, or the widest fraction's width) */
#define ECGVIT_DENOISE_MAX_ROBUST_ITERS 10    /* robust_iters of ecgvit_rloess */
#define ECGVIT_DENOISE_NLM_RUN 15             /* consecutive output samples a lane of the non-local means owns: the unit of tile_runs */
#define ECGVIT_DENOISE_NLM_MAX_THREADS 512    /* lanes of a non-local means workgroup: tile_runs == 0 means one run per lane */
#define ECGVIT_DENOISE_LOESS_LDS 4096         /* f32 samples ecgvit_rloess_tiled keeps in LDS: a tile and two windows */
#define ECGVIT_DENOISE_MAX_TILES 65535        /* tiles per lead of the _tiled entry points (the grid's third dimension) */
/* bytes of `workspace` ecgvit_filtfilt and ecgvit_nlm_sigma need (f64 intermediates, [R][C][max_len + 64]); 0 for unsupported arguments */
int64_t ecgvit_denoise_workspace(int R, int C, int max_len);
/* scipy.signal.filtfilt(b, a, x) with its defaults, per lead: odd extension by padlen = 3 * ntaps samples at each end, a direct-form-II-transposed
 * pass started from zi * x_ext[0], the same pass over the reversed result started from zi * y[-1], reversed again and stripped.  b, a (ntaps each,
 * the shorter padded with zeros; 1 <= ntaps <= ECGVIT_DENOISE_MAX_TAPS; a[0] == 1) and zi (ntaps - 1; scipy.signal.lfilter_zi) are HOST arrays of finite doubles.
 * f64 arithmetic, f32 loads and stores.  min_len: the caller's lower bound of the positive raw_len; min_len <= padlen is refused, where scipy
 * raises (a shorter record that reaches the kernel all the same is left untouched). */
int ecgvit_filtfilt(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                    int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream);
/* sigma[r * C + c] (f64) = the reference's est_noise_std of the lead: res = x; res[i] = (2 res[i] - res[i-1] - res[i+1]) / sqrt(6) for i = 1 .. n-2
 * in place (res[i-1] updated, res[i+1] original); m = median(res); sigma = median |1.4826 (res - m)|.  f64 in the reference's order; both medians
 * are exact order statistics (radix select on the f64 bit pattern; the mean of the two middle values for even n).  scipy's
 * median_abs_deviation subtracts the median of 1.4826 (res - m) once more: exactly 0 for odd n, a rounding of m (1e-16 relative) for even n.
 * Entries of skipped records are not written. */
int ecgvit_nlm_sigma(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                     void *workspace, void *stream);
/* DataPreprocessor.nlm per lead, quirks included (n = 2p + 2 denoises its one middle sample, as the reference's range(p + 1, n - p) does).  p = patch_wd >= 1, W = sch_wd (0 or more than n: n), h = 2 (2p + 1) (scale * sigma[r * C + c])^2.
 * For ii = p + 1 .. n - p - 1:  out[ii] = sum_idx w x[ii + idx] / (sum_idx w + 2.220446049250313e-16) over idx = -(W - 1) .. W - 1 with
 * 0 < ii + idx < n (sample 0 is never a neighbour), w = exp(-d / h), d = sum_{j = -p .. p} (x[ii + j] - x[ii + j + idx])^2 where a pair whose
 * second index lies outside [0, n) contributes 0.  The first p + 1 and the last p samples are copied; a record with n <= 2p + 1 is copied
 * through, and so is a lead with sigma == 0 (or with 1 / h past f32) -- the reference divides 0 by 0 there and returns NaN.
 * f32 arithmetic (1 / h once per lead from the f64 sigma, v_exp_f32).  A lane owns runs of ECGVIT_DENOISE_NLM_RUN consecutive output samples (the last run of a
 * record ends on sample n - p - 1) and adds the shifts in ascending order; d is summed from its 2p + 1 terms at the start of each run and shift
 * and slides within the run (d += new^2 - old^2). */
int ecgvit_nlm_denoise(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len,
                       const double *sigma, double scale, int patch_wd, int sch_wd, void *stream);
/* The robust LOESS baseline the reference subtracts between the low-pass and the non-local means (rloess: loess_1d(x, sig, degree=2,
 * npoints=n)[1] of the `loess` package).  The package is not available, so no fixture could be written by running it: parity with the reference
 * is UNPINNED, and what the tests hold the kernel to is a numpy f64 restatement of the algorithm below (tests/loess_ref.py).
 * Per lead y[0 .. n) at x = 0 .. n - 1, m = min(npoints, n), degree g, for every sample j:
 *   window    the m samples nearest to j, [lo, lo + m): lo = clamp(j - (m - 1) / 2, 0, n - m) for odd m, clamp(j - m / 2, 0, n - m) for even m
 *   weights   d = max(j - lo, lo + m - 1 - j), dw_i = (1 - (|i - j| / d)^3)^3 (the farthest sample has weight 0)
 *   fit       the weighted least-squares polynomial of degree g through the window, weights dw
 *   robust    at most robust_iters times: aerr = |fit - y| over the window, mad = median(aerr) (the mean of the two middle values for even m),
 *             bw = (1 - min((aerr / (6 mad))^2, 1))^2, refit with weights dw bw, bad = bw < 0.34; stop when bad equals the previous
 *             iteration's bad (the first iteration never stops)
 *   result    the last fit's value at j
 * DEFINED HERE, where the reference leaves the result open: (1) for even m the two samples at distance m / 2 tie and the LOWER index enters the
 * window, what a stable sort of the distances gives (the reference's default argsort takes either, by numpy version and CPU; the sample has
 * regression weight 0 but enters the median and `bad`, which moves the result by up to 5e-3 of the amplitude; zheng passes n = fqs = 500, even);
 * (2) mad == 0 (an all-zero lead; below the smallest normal f64 counts as 0) ends the robust loop and the fit it has stands (the reference
 * divides by zero), as the sigma == 0 lead of ecgvit_nlm_denoise is copied through.
 * frac > 0 replaces npoints per record by the reference's force_odd(int(n * frac) - 1) = 2 floor((int(n frac) - 1) / 2) + 1, computed in f64 as
 * Python computes it.  degree: 1 or 2; robust_iters: 0 (the plain LOESS) .. ECGVIT_DENOISE_MAX_ROBUST_ITERS; npoints (frac == 0), or the fraction's width of a record of
 * max_len samples: at most ECGVIT_DENOISE_MAX_POINTS; npoints, and the fraction's width of a record of min_len samples: at least degree + 2.  min_len: the caller's
 * lower bound of the positive raw_len, at least degree + 2 (a record whose window is narrower or wider all the same is left untouched).
 * subtract == 0 writes the baseline, 1 writes x - baseline (the difference in f64, rounded once); out == x works in both.
 * iters (nullable): bytes [R][C][max_len], the robust iterations run at sample j of lead c of the launch's r-th record at
 * iters[(r * C + c) * max_len + j]; other bytes are not written.
 * f64 arithmetic without contraction: s = (i - j) (1 / d); eight moment sums (sum w s^k, k = 0 .. 4; sum w s^k y, k = 0 .. 2), window sample
 * lo + l + 64 v in slot v of lane l, a lane adds its slots in ascending order, the wave adds lanes by the butterfly 32, 16, .. 1; the normal
 * equations by elimination without pivoting; the value at j is the constant coefficient.  The median is an exact order statistic. */
int ecgvit_rloess(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                  int max_len, int npoints, double frac, int degree, int robust_iters, int subtract, int8_t *iters, void *stream);

/* ---- records longer than ECGVIT_DENOISE_MAX_LEN samples (Holter length): the same stages with max_len up to ECGVIT_DENOISE_MAX_LEN_TILED.
 * Additive entry points: the ABI version stays 6.  The store is addressed as above; every per-record index that multiplies by max_len is 64-bit.
 * The entry points above keep their cap and their behaviour; these are opt-in and run short records too.
 * ecgvit_denoise_workspace_long, ecgvit_filtfilt_long, ecgvit_nlm_sigma_long: the formula, the arguments and THE KERNELS of
 * ecgvit_denoise_workspace, ecgvit_filtfilt and ecgvit_nlm_sigma (one launcher each, two caps): a record's bits are the same from either entry
 * point.  Both kernels stage the lead through LDS in chunks and keep their f64 intermediates in `workspace`; the recurrence is walked by one
 * lane (a block-parallel IIR would change the bits). */
int64_t ecgvit_denoise_workspace_long(int R, int C, int max_len);
int ecgvit_filtfilt_long(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                         int max_len, const double *b, const double *a, const double *zi, int ntaps, void *workspace, void *stream);
int ecgvit_nlm_sigma_long(const float *x, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len, double *sigma,
                          void *workspace, void *stream);
/* ecgvit_nlm_denoise tiled along time: grid (R, C, tiles), a workgroup owns tile_runs consecutive runs of ECGVIT_DENOISE_NLM_RUN output samples of one lead
 * (tile_runs == 0: ECGVIT_DENOISE_NLM_MAX_THREADS, one run per lane of a workgroup that wide; more runs than the longest record holds are clamped to that).  The run
 * decomposition is ecgvit_nlm_denoise's: run k starts at p + 1 + ECGVIT_DENOISE_NLM_RUN k, the last run is moved back to end on n - p - 1, a lane owns whole runs and
 * adds the shifts in ascending order, d is summed afresh at the start of each (run, shift) and slides within the run.  A lane's own window is
 * loaded from global memory; the neighbour side is streamed through LDS in ascending chunks of 256 shifts, double-buffered.
 * CONTRACT: the order of every sum is a function of n, p and W alone, so the output is bit-identical to ecgvit_nlm_denoise for every
 * n <= ECGVIT_DENOISE_MAX_LEN and every tile_runs.
 * out == x is REFUSED (ECGVIT_EINVAL): a workgroup reads samples that another workgroup writes, where ecgvit_nlm_denoise loads the lead before
 * its first store.  Also refused: tile_runs < 0, patch_wd > ECGVIT_DENOISE_MAX_LEN_TILED, and a tile_runs so small that max_len needs more than ECGVIT_DENOISE_MAX_TILES tiles. */
int ecgvit_nlm_denoise_tiled(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int max_len,
                             const double *sigma, double scale, int patch_wd, int sch_wd, int tile_runs, void *stream);
/* ecgvit_rloess tiled along time: grid (R, C, tiles), a workgroup owns tile_samples consecutive output samples [j0, j0 + tile_samples) and
 * loads x[max(0, j0 - m) .. min(n, j0 + tile_samples + m)) into an LDS array of ECGVIT_DENOISE_LOESS_LDS f32 (tile_samples == 0: ECGVIT_DENOISE_LOESS_LDS - 2 * ECGVIT_DENOISE_MAX_POINTS, which fits with two
 * windows of the widest width).  The per-sample wave code is ecgvit_rloess's, unchanged (window placement, even-tie rule, moment sums,
 * elimination, bit-by-bit median, `iters` bytes), and a sample's arithmetic reads only its window.
 * CONTRACT: the output and `iters` are bit-identical to ecgvit_rloess for every n <= ECGVIT_DENOISE_MAX_LEN and every tile_samples.
 * Refused: tile_samples < 0; tile_samples + 2 * (the launch's widest window, at most max_len) > ECGVIT_DENOISE_LOESS_LDS; more than ECGVIT_DENOISE_MAX_TILES tiles for max_len;
 * out == x (as above). */
int ecgvit_rloess_tiled(const float *x, float *out, const int64_t *src_off, int64_t lead_stride, const int32_t *raw_len, int R, int C, int min_len,
                        int max_len, int npoints, double frac, int degree, int robust_iters, int subtract, int8_t *iters, int tile_samples,
                        void *stream);

/* ------------------------------------------------------------------------------------------------
 * Fourier resampling of a record store to another length (resample.py; the reference's export stage, preprocess/data_export.py:202-215:
 * wfdb.processing.resample_sig(sig, fqs, 250) per lead, which reduces to scipy.signal.resample(x, num = int(n * fs_target / fs))).  Parity is
 * pinned at the scipy call; the wfdb wrapper and its length rule are restated (resample.resampled_length), not executed.  Additive entry points:
 * the ABI version stays 6.
 * The one stage whose output has another shape than its input: the source is addressed as ecgvit_fit_moments addresses it (lead c of record r =
 * n_in f32 samples at x + src_off[r] + c * src_stride), the destination by a table of its own (n_out f32 samples at out + dst_off[r] +
 * c * dst_stride; src_off, dst_off int64 [R], device arrays); every record of a call has the same n_in and the same n_out: the caller groups a
 * ragged store by length.  A record starts at any 4-byte address; out must not overlap x.  1 <= n_in, n_out <= ECGVIT_RESAMPLE_MAX_LEN; all per-record indexing
 * is 64-bit.  NaN input is not supported (wfdb interpolates NaN before it resamples).
 * ALGORITHM, per record:
 *   pairing   C is even; leads 2p and 2p + 1 are the real and the imaginary part of one complex f64 sequence z of n_in samples.  The resample is
 *             linear and the spectrum rule below is scipy's rule for complex input, so resample(x_a + i x_b) = resample(x_a) + i resample(x_b):
 *             one transform serves two leads and no spectrum separation is needed.  The two leads meet only in rounding (tests: 1e-12 of the
 *             record's largest sample).
 *   forward   X = DFT(z), X[k] = sum_j z[j] exp(-2 pi i j k / n_in)
 *   spectrum  N = min(n_in, n_out); Y has n_out bins, zero but for Y[m] = X[m], m = 0 .. N/2, and Y[n_out - m] = X[n_in - m],
 *             m = 1 .. N - N/2 - 1 (integer halves).  For even N: downsampling (n_out < n_in) Y[N/2] += X[n_in - N/2]; upsampling (n_in < n_out)
 *             Y[N/2] is halved and Y[n_out - N/2] set to the same value.  Every bin is multiplied by 1 / n_in (the inverse transform's
 *             1 / n_out times scipy's n_out / n_in).
 *   inverse   y[j] = sum_m Y[m] exp(+2 pi i j m / n_out); re y -> lead 2p, im y -> lead 2p + 1, each rounded once to f32.
 *   twiddles  tw_in[k] = exp(-2 pi i k / n_in), k < n_in, and tw_out[k] = exp(+2 pi i k / n_out), k < n_out: (re, im) f64 pairs in DEVICE memory,
 *             16-byte aligned, made by the caller (resample.py: numpy on the host).  The kernels compute no sine or cosine: every root of unity,
 *             those of the small transforms included, is a table entry, so the bits do not depend on a device math library.
 *   plan      a transform of length n is a sequence of mixed-radix Stockham (autosort, out-of-place) passes, one launch each over all records and
 *             lead pairs of the call, ping-pong between the two halves of `workspace`.  The radices are a pure function of n: the built radices
 *             25, 16, 8, 5, 4, 3, 2 in this order, each for as long as it divides what is left, then every remaining prime factor in ascending
 *             order, with multiplicity.  The built radices run in registers (16 and 8 as 4 x 4 and 4 x 2, 25 as 5 x 5); any other radix r runs
 *             one generic pass: a thread per output, a loop over its r inputs.  With r = n that pass is the dense DFT, so a prime length works,
 *             at n^2 complex multiply-adds per lead pair and direction instead of n log n (n = 32 771, prime: 1.1e9; the chirp route below is
 *             the n log n form, through ecgvit_resample_chirp).  A generic radix above ECGVIT_RESAMPLE_MAX_GENERIC is refused: its pass would hold the device for
 *             minutes.
 *             Pass with radix r after passes of product Ns, butterfly j < n / r, k = j mod Ns: v[q] = in[j + q n / r] tw[q k n / (Ns r)],
 *             u = DFT_r(v), out[(j - k) r + k + p Ns] = u[p].
 * Each pass reads and writes 16 bytes per complex element: an HBM stream of 32 bytes per element, pack and unpack 8 + 16 each.
 * No atomics; every sum runs in an order fixed by (n_in, n_out): a record's output has the same bits in a rectangle, a ragged store, a subset or
 * a chunk, alone or in a batch.
 * ------------------------------------------------------------------------------------------------ */
#define ECGVIT_RESAMPLE_MAX_LEN 33554432     /* n_in, n_out and the M of a chirp side: 1 << 25 samples, ECGVIT_DENOISE_MAX_LEN_TILED */
#define ECGVIT_RESAMPLE_MAX_CHIRP 16777216   /* a length on the chirp route: 1 << 24 samples, so that its M stays within ECGVIT_RESAMPLE_MAX_LEN */
#define ECGVIT_RESAMPLE_MAX_GENERIC 65536    /* the widest generic radix (prime factor) that is launched */
#define ECGVIT_RESAMPLE_MAX_GRID_Y 65535     /* R * (C / 2) of one call: the grid's second dimension holds record x lead pair */
/* radices[0 .. count) = the plan of a length n, 1 <= n <= ECGVIT_RESAMPLE_MAX_LEN -> count (their product is n; n == 1 has the empty plan, count 0; a prime
 * has the plan { n }); -1 for n out of range or more radices than `cap`.  Host only: nothing is launched. */
int ecgvit_resample_plan(int n, int *radices, int cap);
/* bytes of `workspace` ecgvit_resample needs: two buffers of R * (C / 2) * max(n_in, n_out) complex f64; 0 for unsupported arguments (C odd,
 * R * C / 2 > ECGVIT_RESAMPLE_MAX_GRID_Y, a length out of range or with a generic radix above ECGVIT_RESAMPLE_MAX_GENERIC) */
int64_t ecgvit_resample_workspace(int R, int C, int n_in, int n_out);
/* launches: pack, the passes of n_in, the spectrum map, the passes of n_out, unpack.  n_in == n_out runs the round trip (resample.py copies
 * instead, as wfdb does).  Unsupported arguments (as above, a null or misaligned pointer) return ECGVIT_EINVAL and launch nothing. */
int ecgvit_resample(const float *x, float *out, const int64_t *src_off, int64_t src_stride, const int64_t *dst_off, int64_t dst_stride, int R, int C,
                    int n_in, int n_out, const double *tw_in, const double *tw_out, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The chirp route (Bluestein's algorithm, the chirp-z transform): the exact DFT of ANY length n <= ECGVIT_RESAMPLE_MAX_CHIRP at O(n log n), as one circular
 * convolution of a smooth length M run by the passes above.  Additive and opt-in (resample.py: `chirp=`): ecgvit_resample, its plan and its
 * workspace query are unchanged, and the ABI version stays 6.  A side of a resample (the forward transform of n_in, the inverse transform of
 * n_out) either runs its plan as above ("plain") or is transformed AS A WHOLE by the chirp route; the two sides choose independently.
 * ALGORITHM, for a transform of length n and sign s (-1: the forward side, +1: the inverse side), X[k] = sum_j z[j] exp(s 2 pi i j k / n):
 *   chirp     w[j] = exp(s i pi j^2 / n), j < n: (re, im) f64 pairs in DEVICE memory, 16-byte aligned, made by the caller as
 *             cos / sin(pi ((j j) mod 2 n) / n) with the square and the reduction in 64-bit integers (resample.py: numpy on the host).  No
 *             device trigonometry, as above.  j k = (j^2 + k^2 - (k - j)^2) / 2 gives X[k] = w[k] sum_j (z[j] w[j]) conj(w[k - j]).
 *   length    M = the smallest integer >= 2 n - 1 of the form 2^a 3^b 5^c (ecgvit_resample_chirp_length), so the plan of M holds built radices
 *             only; n <= ECGVIT_RESAMPLE_MAX_CHIRP keeps M <= ECGVIT_RESAMPLE_MAX_LEN, the cap of the passes.
 *   operand   a[j] = z[j] w[j], j < n; a[j] = 0, n <= j < M.
 *   filter    b[j] = conj(w[j]), j < n; b[M - j] = conj(w[j]), 1 <= j < n; b = 0 elsewhere.  filter = DFT_M(b) / M, computed on the device
 *             once per (n, s) by the same passes (ecgvit_resample_chirp_filter) and passed to every launch of that length.
 *   result    c = conj(DFT_M(conj(DFT_M(a) filter))) (the circular convolution of a and b), X[k] = w[k] c[k], k < n.
 *   tables    the inverse M-transform is the forward one between two conjugations, so a length M needs ONE twiddle table,
 *             tw_M[k] = exp(-2 pi i k / M), k < M, whatever s is, shared by every n that maps to that M.
 * KERNELS (complex f64, no atomics; transforms of a chirp side live at stride M in the workspace), and what is fused:
 *   pack      forward side: the f32 lead pair -> a, the chirp multiply and the zero fill up to M folded into the pack (one launch over M).
 *   product   A[j] <- conj(A[j] filter[j]), j < M, in place: the one sweep of its own (32 bytes per element) between the two runs of passes.
 *   post      X[k] = w[k] conj(D[k]), D = DFT_M(conj(A filter)): no launch of its own.  Forward side: folded into the spectrum map's loads
 *             (the map reads bin k as w_in[k] conj(D[k])).  Inverse side: folded into the unpack, rounded once to f32.
 *   pre       inverse side: the spectrum map's output Y[m] / n_in, times w_out[m], with the zero fill n_out <= m < M: folded into the spectrum
 *             map's stores (one launch over M).
 * Every element of an operand up to M is WRITTEN by the pack or the map before a pass reads it: the content of `workspace` is never assumed.
 * Launches of a chirp side: 2 passes(M) + 1 beside pack / map / unpack.  Every sum's order is fixed by (n_in, n_out, route of each side): a
 * record keeps the same bits in every store form.  The two routes of one length agree within rounding, not bit for bit.
 * ------------------------------------------------------------------------------------------------ */
/* M of a length n: the smallest 2^a 3^b 5^c >= 2 n - 1; -1 for n < 1 or n > ECGVIT_RESAMPLE_MAX_CHIRP.  Host only. */
int ecgvit_resample_chirp_length(int n);
/* bytes of `workspace` ecgvit_resample_chirp needs: two buffers of R * (C / 2) * max(side lengths) complex f64, where a chirp side (flag != 0)
 * counts its M and a plain side its n; 0 for anything refused (as ecgvit_resample_workspace for a plain side; n > ECGVIT_RESAMPLE_MAX_CHIRP on a chirp side) */
int64_t ecgvit_resample_chirp_workspace(int R, int C, int n_in, int n_out, int chirp_in, int chirp_out);
/* filter[0 .. M) = DFT_M(b) / M for the chirp table `chirp` of n entries (either sign), M == ecgvit_resample_chirp_length(n), tw_M the table of
 * M above; `workspace`: 2 M complex f64 (32 M bytes), every element written before it is read.  All pointers device memory, 16-byte aligned.
 * Launches: the fill of b, the passes of M, the scaling.  Null or misaligned pointers, n out of range, another M: ECGVIT_EINVAL, no launch. */
int ecgvit_resample_chirp_filter(const double *chirp, int n, int M, const double *tw_M, double *filter, void *workspace, void *stream);
/* ecgvit_resample with a route per side.  chirp_in / filter_in both null: the input side is plain and tw_in is the table of n_in, as in
 * ecgvit_resample; both non-null: the input side takes the chirp route, chirp_in = w of (n_in, -1), filter_in its filter, and tw_in is the table
 * of M_in, exp(-2 pi i k / M_in).  chirp_out / filter_out likewise with (n_out, +1): plain takes tw_out = exp(+2 pi i k / n_out), chirp takes
 * tw_out = exp(-2 pi i k / M_out).  Both sides plain runs ecgvit_resample's launches and gives its bits.  `workspace`:
 * ecgvit_resample_chirp_workspace bytes.  Everything is checked on the host; a null or misaligned pointer, half of a chirp / filter pair, a
 * chirp side above ECGVIT_RESAMPLE_MAX_CHIRP samples, a plain side ecgvit_resample refuses: ECGVIT_EINVAL, and nothing is launched. */
int ecgvit_resample_chirp(const float *x, float *out, const int64_t *src_off, int64_t src_stride, const int64_t *dst_off, int64_t dst_stride, int R,
                          int C, int n_in, int n_out, const double *tw_in, const double *tw_out, const double *chirp_in, const double *filter_in,
                          const double *chirp_out, const double *filter_out, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ECGVIT_HIP_H */
