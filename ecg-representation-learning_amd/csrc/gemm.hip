// The GEMM front door: plan_gemm decides, before anything is launched, whether a call is valid and how it runs -- kernel family, epilogue
// instantiation, store form, tile walk, split-K factor, grid and post-passes.  Every extern "C" GEMM entry point is a thin layer over it:
// ecgvit_gemm / ecgvit_gemm_rowpitch run the plan, ecgvit_gemm_kernel / ecgvit_gemm_workspace report it, so asking and running agree.
#include "gemm_plan.h"
#include <algorithm>

namespace {

bool is_f8(int t) { return t == ECGVIT_FP8_E4M3 || t == ECGVIT_BF8_E5M2; }
bool al16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
bool abc_al16(const ecgvit_gemm_desc *d) { return al16(d->A) && al16(d->B) && al16(d->C); }
bool fits31(int64_t v) { return v < (1ll << 31); }
int ceil_div(int64_t a, int b) { return (int)((a + b - 1) / b); }

// aux (GELU / GELU_BWD / MUL_AUX) and residual present, 16-B aligned, whole 8-element rows
bool aux_res_ok(const ecgvit_gemm_desc *d) {
    if ((d->epilogue & (ECGVIT_EPI_GELU | ECGVIT_EPI_GELU_BWD | ECGVIT_EPI_MUL_AUX)) && (!d->aux || d->ldaux % 8 || !al16(d->aux))) return false;
    return !(d->epilogue & ECGVIT_EPI_RESIDUAL) || (d->residual && d->ldr % 8 == 0 && al16(d->residual));
}

template <typename Go> auto with_nt_sets(const ecgvit_gemm_desc *d, Go &&go) {
    if (d->dtype == ECGVIT_FP8_E4M3) return go(epi_sets::E4m3{});
    if (d->dtype == ECGVIT_BF8_E5M2) return go(epi_sets::E5m2{});
    return d->out_dtype == ECGVIT_BF16 ? go(epi_sets::Bf16{}) : go(epi_sets::F32Out{});
}
bool nt_own_body(const ecgvit_gemm_desc *d) { return with_nt_sets(d, [&](auto sets) { return epi_in(sets, d->epilogue); }); }

// the persistent A . B^T kernel (gemm_nt.hip): M >= 2048, K-contiguous operands, 32-bit byte offsets
bool nt_ok(const ecgvit_gemm_desc *d) {
    const bool f8 = is_f8(d->dtype);
    const int epi = d->epilogue;
    if (d->layout != ECGVIT_GEMM_NT || !(d->dtype == ECGVIT_BF16 || f8)) return false;
    if (d->batch1 != 1 || d->batch2 != 1) return false;
    if (d->M < 2048 || d->N < 128 || d->N % 8 != 0) return false;
    if (f8 ? (d->K % 128 != 0 || d->K < 384 || d->lda % 16 != 0 || d->ldb % 16 != 0 || d->out_dtype != ECGVIT_BF16) : (d->K % 64 != 0 || d->K < 192)) return false;
    const int es = f8 ? 1 : 2;
    if (!fits31((int64_t)d->M * d->lda * es + 65536 * d->lda) || !fits31((int64_t)d->N * d->ldb * es + 65536 * d->ldb)) return false;
    const int64_t esz = d->out_dtype == ECGVIT_BF16 ? 2 : 4, rows = (int64_t)d->M + 256;   // epilogue offsets are 32-bit byte offsets
    if (!fits31(rows * d->ldc * esz) || !fits31(rows * d->ldr * 2) || !fits31(rows * d->ldaux * 2)) return false;
    if (!(epi & ECGVIT_EPI_NO_OUT) && !d->C) return false;
    // no-output form and the e4m3 saved tensor: the sets with a body of their own only
    if ((epi & (ECGVIT_EPI_NO_OUT | ECGVIT_EPI_AUX8)) && !nt_own_body(d)) return false;
    if ((epi & ECGVIT_EPI_AUX8) && (!d->aux || d->ldaux % 8 || reinterpret_cast<uintptr_t>(d->aux) % 8)) return false;
    if ((epi & ECGVIT_EPI_QUANT_OUT) &&
        (!f8 || !d->q8_out || !d->q8_scale || !d->q8_amax || d->ldq8 % 8 || reinterpret_cast<uintptr_t>(d->q8_out) % 8 ||
         (d->q8_format != ECGVIT_FP8_E4M3 && d->q8_format != ECGVIT_BF8_E5M2) || !fits31(rows * d->ldq8)))
        return false;
    if ((epi & ECGVIT_EPI_COLSUM) &&   // fused column sums: 8 bytes per column and 256-row tile of partial sums
        (d->out_dtype != ECGVIT_BF16 || !d->workspace || !d->colsum_out || d->workspace_bytes < (int64_t)8 * ceil_div(d->M, GEMM_NT_TILE) * d->N))
        return false;
    return true;
}

// the streaming split-K weight-gradient kernels (gemm_wgrad.hip): both extents whole 256-tiles, a long reduction
bool wgrad_ok(const ecgvit_gemm_desc *d) {
    const bool f8 = is_f8(d->dtype);
    if (d->layout != ECGVIT_GEMM_TN || !(d->dtype == ECGVIT_BF16 || f8) || d->batch1 != 1 || d->batch2 != 1) return false;
    if (d->epilogue & ~(ECGVIT_EPI_BIAS | ECGVIT_EPI_ACCUM)) return false;
    if (d->K < 4096 || d->M % 256 != 0 || d->N % 256 != 0) return false;
    const int es = f8 ? 1 : 2;
    if (f8 && (d->out_dtype != ECGVIT_F32 || d->lda % 16 || d->ldb % 16 || !d->A || !d->B || !al16(d->A) || !al16(d->B)))
        return false;   // 8-bit operands: f32 output, 16-B aligned rows (one DMA lane = 16 bytes of a row)
    return fits31((int64_t)d->K * d->lda * es + 65536 * d->lda) && fits31((int64_t)d->K * d->ldb * es + 65536 * d->ldb);
}

// split-K factor of the 128^2 kernel's TN products
int choose_splits(const ecgvit_gemm_desc *d, int ntile) {
    if (d->layout != ECGVIT_GEMM_TN) return 1;
    const int ksteps = ceil_div(d->K, GEMM_BK);
    int s = (768 + ntile - 1) / ntile;  // aim for ~3 waves of blocks over 256 CUs
    s = std::min(s, std::max(1, ksteps / 8));  // keep >= 8 K-steps per split
    return std::max(1, std::min(s, 64));
}

// split-K factor of the weight-gradient kernels
int choose_splits2(const ecgvit_gemm_desc *d, int ntile) {
    if (d->layout != ECGVIT_GEMM_TN) return 1;
    const int ksteps = ceil_div(d->K, GEMM_BK);
    // one block per CU: fill ONE round of the 256 CUs (never 2.1 rounds); a multiple of 8 slices lets each XCD own whole K-slices
    int s = 256 / ntile;
    // a multiple of 8 slices lets each XCD own whole K-slices (best L2 locality), but only if the rounding leaves < 7 % of the CUs idle:
    // 27 tiles x 8 slices = 216 blocks wastes 16 % of the chip for the whole launch, 27 x 9 = 243 (XCD-contiguous order) does not
    if (s >= 8 && (s & ~7) * ntile * 100 >= s * ntile * 93) s &= ~7;
    if (s < 1) s = 1;
    // tiles_per_workgroup (launches that share the GPU with RCCL kernels) does NOT change the slicing here.  Three times as many,
    // shorter slices would bound the tail of a block that finds its CU held, but they cost every launch: measured inside the step on
    // a 1-rank RCCL group (bench.py --single-rank-collectives, profiles/r02_dp_single_rank.txt) +2.3 ms of gemm_wgrad and +1.1 ms of
    // split-K reduce per step, against the ~8 % of the backward during which a bucket's all-reduce actually holds CUs.
    s = std::min(s, std::max(1, ksteps / 16));   // keep >= 16 K-steps per slice
    return std::max(1, std::min(s, 64));
}

int64_t slab_bytes(const ecgvit_gemm_desc *d, int splits) { return splits > 1 ? (int64_t)splits * d->M * d->N * 4 : 0; }
int wgrad_splits(const ecgvit_gemm_desc *d) { return choose_splits2(d, (d->M / GEMM_WGRAD_TILE) * (d->N / GEMM_WGRAD_TILE)); }
// the largest factor <= sp whose slabs fit the caller's workspace
int fit_splits(const ecgvit_gemm_desc *d, int sp) {
    while (sp > 1 && slab_bytes(d, sp) > d->workspace_bytes) --sp;
    return sp;
}

// Workspace a TN call needs for its preferred split-K factor.  A bf16 TN shape reports the larger need of its two split-K families, so a
// buffer sized once per shape serves every epilogue and pointer set of it (the engine sizes `ws` so).
int64_t preferred_workspace(const ecgvit_gemm_desc *d) {
    const int64_t w2 = wgrad_ok(d) ? slab_bytes(d, wgrad_splits(d)) : 0;
    if (is_f8(d->dtype) && d->layout == ECGVIT_GEMM_TN) return w2;
    if (d->dtype != ECGVIT_BF16 || d->layout != ECGVIT_GEMM_TN) return 0;
    const int ntile = ceil_div(d->M, GEMM_BF16_TILE) * ceil_div(d->N, GEMM_BF16_TILE);
    return std::max(slab_bytes(d, choose_splits(d, ntile)), w2);
}

bool f32_args_ok(const ecgvit_gemm_desc *d) {
    if (d->out_dtype != ECGVIT_F32 || d->M <= 0 || d->N <= 0 || d->K < 0 || d->batch1 < 1 || d->batch2 < 1) return false;
    const int64_t nz = (int64_t)d->batch1 * d->batch2;   // (residual / aux are not batched)
    return nz <= 65535 && !(nz > 1 && (d->epilogue & (ECGVIT_EPI_GELU | ECGVIT_EPI_GELU_BWD | ECGVIT_EPI_RESIDUAL | ECGVIT_EPI_DROPOUT)));
}

bool bf16_args_ok(const ecgvit_gemm_desc *d) {
    if (d->out_dtype != ECGVIT_BF16 && d->out_dtype != ECGVIT_F32) return false;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0 || d->batch1 != 1 || d->batch2 != 1) return false;
    if (d->N % 8 != 0 || d->lda % 8 != 0 || d->ldb % 8 != 0 || d->ldc % 8 != 0 || !abc_al16(d)) return false;
    const bool a_kc = d->layout != ECGVIT_GEMM_TN, b_kc = d->layout == ECGVIT_GEMM_NT;
    if ((a_kc || b_kc) && d->K % 8 != 0) return false;      // K-contiguous operands move 8-element chunks
    if (!a_kc && d->M % 8 != 0) return false;
    if (d->out_dtype == ECGVIT_F32 &&
        (d->epilogue & (ECGVIT_EPI_GELU | ECGVIT_EPI_GELU_BWD | ECGVIT_EPI_MUL_AUX | ECGVIT_EPI_RESIDUAL | ECGVIT_EPI_DROPOUT)))
        return false;
    return !((d->epilogue & ECGVIT_EPI_BIAS) && !al16(d->bias)) && aux_res_ok(d);
}

// 8-bit A . B^T operands (the large kernel only: no small-shape fallback)
bool f8_nt_args_ok(const ecgvit_gemm_desc *d) {
    if (!d->A || !d->B || (!d->C && !(d->epilogue & ECGVIT_EPI_NO_OUT)) || !abc_al16(d) || d->ldc % 8 != 0) return false;
    return !((d->epilogue & ECGVIT_EPI_BIAS) && (!d->bias || !al16(d->bias))) && aux_res_ok(d);
}

// the stand-alone column sum (ecgvit_colsum) over the stored output
bool colsum_args_ok(const ecgvit_gemm_desc *d) {
    return d->M > 0 && d->N > 0 && d->N % 8 == 0 && d->ldc % 8 == 0 && (d->out_dtype == ECGVIT_F32 || d->out_dtype == ECGVIT_BF16) &&
           d->workspace_bytes >= ecgvit_colsum_workspace(d->M, d->N);
}

// the kernel family that takes the call, ECGVIT_KERNEL_NONE if none does
int family(const ecgvit_gemm_desc *d) {
    const int dt = d->dtype;
    if (dt == ECGVIT_F32) return f32_args_ok(d) && d->layout >= ECGVIT_GEMM_NT && d->layout <= ECGVIT_GEMM_TN ? ECGVIT_KERNEL_GEMM_F32 : ECGVIT_KERNEL_NONE;
    if (dt == ECGVIT_BF16) {
        if (!bf16_args_ok(d) || d->layout < ECGVIT_GEMM_NT || d->layout > ECGVIT_GEMM_TN) return ECGVIT_KERNEL_NONE;
        return nt_ok(d) ? ECGVIT_KERNEL_GEMM_NT : wgrad_ok(d) ? ECGVIT_KERNEL_GEMM_WGRAD : ECGVIT_KERNEL_GEMM_BF16;
    }
    if (is_f8(dt) && d->layout == ECGVIT_GEMM_TN)   // 8-bit weight gradients dW = dY8^T . X8 (A in `dtype`, B e4m3, f32 output)
        return d->C && al16(d->C) && d->ldc % 4 == 0 && wgrad_ok(d) ? ECGVIT_KERNEL_GEMM_WGRAD : ECGVIT_KERNEL_NONE;
    if (is_f8(dt)) return f8_nt_args_ok(d) && nt_ok(d) ? ECGVIT_KERNEL_GEMM_NT : ECGVIT_KERNEL_NONE;
    return ECGVIT_KERNEL_NONE;
}

void plan_nt(GemmPlan &p, const ecgvit_gemm_desc *d) {
    using namespace epi_sets;
    const int epi = d->epilogue;
    p.tiles_m = ceil_div(d->M, GEMM_NT_TILE);
    p.tiles_n = ceil_div(d->N, GEMM_NT_TILE);
    const int ntile = p.tiles_m * p.tiles_n;
    // Built-in tile walk: column groups of 6 n-tiles (m-major inside a group).  Measured inside the train step against the plain
    // n-fastest order (profiles/r02_raster_step.txt): the same step time (+-0.02 %) with 13 % fewer bytes
    // fetched from beyond L2 per launch (1.08 -> 0.94 GB); groups of 3 fetch 0.97 GB at -0.1 %, groups of 4 cost 0.6 % of the step.
    // Up to 8 n-tiles (N <= 2048: the FFN-wide products of EcgVit-small) stay ONE group -- a 6 + 2 split costs that step 0.9 % (round 4).
    p.group = p.tiles_n <= 8 ? p.tiles_n : 6;
    // persistent (one workgroup per CU, static shares) unless the caller asks for dispatcher-balanced chunks of ~k tiles
    const int tpw = d->tiles_per_workgroup;
    p.grid = dim3((unsigned)(tpw > 0 ? std::max(std::min(ntile, 256), (ntile + tpw - 1) / tpw) : std::min(ntile, 256)));
    p.body = GemmBody::NT;
    p.fl = nt_own_body(d) ? epi : -1;
    const bool alpha1 = d->alpha == 1.f && !d->scale_a && !d->scale_b;   // (the four-wave body has no alpha)
    const int64_t out_bytes = (int64_t)d->M * d->N * 2;
    if (is_f8(d->dtype)) {
        // plain 8-bit products whose bf16 output does not fit the 256-MB Infinity Cache (EcgVit-large: the QKV forward's 788 MB) store it non-temporally, as
        // the bf16 QKV forward does since round 3: written through L2 the output evicts the operand panels the tile's neighbours are about to re-read
        // (profiles/r06_fp8_nt_stores.txt at 256 x 501 token rows, default -> non-temporal: QKV forward K = 1024, 752 MB: 403.8 -> 350.5 us; the 250-MB outputs: K = 1024
        // 145.5 -> 133.8, K = 3072 323.0 -> 338.1, K = 4096 411.8 -> 422.9: a long main loop re-reads its panels from L2 often enough to want the cache's help)
        p.nt_stores = epi == 0 && (out_bytes > (320ll << 20) || (out_bytes > (240ll << 20) && d->K <= 1024));
    } else if (d->out_dtype == ECGVIT_BF16 && epi == 0) {
        // plain products.  K >= 1536 (the QKV and FFN-up input gradients): the four-wave body (alpha 1 only).
        // Outputs that do not fit the 256 MB Infinity Cache (QKV forward: 592 MB) are stored non-temporally: written through L2 they
        // evict the operand panels the tile's neighbours are about to re-read (main loop 3,020 -> 2,620 cycles per K-tile, launch
        // -6...-10 %); smaller outputs (197 MB) are absorbed by the cache and nt costs them 2-3 % (profiles/r03_gemm_4w.txt)
        p.nt_stores = out_bytes > (256ll << 20);
        if (d->K >= 1536 && alpha1) p.body = GemmBody::NT4W;
    } else if (d->out_dtype == ECGVIT_BF16 && (epi & ~D) == LIN && d->K >= 768 && alpha1) {
        // the two residual launches (bias + residual [+ dropout]: attn-out and FFN-down forward) with K >= 768: the four-wave body as well --
        // its shorter main loop outweighs the one-wave epilogue (launch -2 % at K = 768, -3 % at K = 3072; step +0.2...0.3 %)
        // (the FFN-down input gradient's body -- x aux, column sums -- measured 1,044 us on this body against 696: 288 B of spills, one wave's VALU)
        p.body = GemmBody::NT4W;
    }
}

void plan_wgrad(GemmPlan &p, const ecgvit_gemm_desc *d) {
    p.body = is_f8(d->dtype) ? GemmBody::WGRAD8 : GemmBody::WGRAD;
    p.tiles_m = d->M / GEMM_WGRAD_TILE;
    p.tiles_n = d->N / GEMM_WGRAD_TILE;
    const int ksteps = ceil_div(d->K, GEMM_BK);
    p.k_per_split = ksteps * GEMM_BK;
    const int sp = d->workspace ? fit_splits(d, wgrad_splits(d)) : 1;
    if (sp > 1) {
        p.splits = sp;
        p.k_per_split = ((ksteps + sp - 1) / sp) * GEMM_BK;
        if (is_f8(d->dtype)) p.k_per_split = ((ceil_div(d->K, 128) + sp - 1) / sp) * 128;   // 8-bit K-tiles are 128 token rows deep
    }
    p.grid = dim3((unsigned)(p.tiles_m * p.tiles_n * p.splits));
}

void plan_bf16(GemmPlan &p, const ecgvit_gemm_desc *d) {
    p.body = GemmBody::BF16;
    p.tiles_m = ceil_div(d->M, GEMM_BF16_TILE);
    p.tiles_n = ceil_div(d->N, GEMM_BF16_TILE);
    const int ntile = p.tiles_m * p.tiles_n, ksteps = ceil_div(d->K, GEMM_BK);
    p.k_per_split = ksteps * GEMM_BK;
    if (d->workspace && d->layout == ECGVIT_GEMM_TN) {
        const int sp = fit_splits(d, choose_splits(d, ntile));
        if (sp > 1 && ((int64_t)d->M * d->N) % 4 == 0 && !(d->epilogue & ~(ECGVIT_EPI_BIAS | ECGVIT_EPI_ACCUM))) {
            p.splits = sp;
            p.k_per_split = ((ksteps + sp - 1) / sp) * GEMM_BK;
        }
    }
    p.grid = dim3((unsigned)(ntile * p.splits));
}

GemmPlan plan_gemm(const ecgvit_gemm_desc *d, int mask_row_pitch) {
    GemmPlan p;
    if (!d) return p;
    p.workspace = preferred_workspace(d);
    if (mask_row_pitch < 1 || (int64_t)d->N * mask_row_pitch >= (1ll << 31)) return p;
    p.mask_row_pitch = mask_row_pitch;
    const int epi = d->epilogue;
    // the no-output form and the e4m3 saved tensor exist on the large A . B^T kernel only (its bodies in epi_sets)
    if ((epi & (ECGVIT_EPI_NO_OUT | ECGVIT_EPI_AUX8)) && !nt_ok(d)) return p;
    if ((epi & ECGVIT_EPI_DROPOUT) && d->dropout_p > 0.f && d->out_dtype == ECGVIT_BF16 && dropout_threshold8(d->dropout_p) == 0u)
        return p;   // 16-bit outputs draw 8 bits per element: 0 < p < 1/512 would silently round to no dropout
    ecgvit_gemm_desc g = *d;
    if (epi & ECGVIT_EPI_COLSUM) {
        if (!d->colsum_out || !d->workspace || d->batch1 != 1 || d->batch2 != 1) return p;
        if (!nt_ok(d)) {   // generic path: the product without the flag, then the stand-alone column sum over the stored output
            if (!colsum_args_ok(d)) return p;
            g.epilogue &= ~ECGVIT_EPI_COLSUM;
            p.colsum = true;
        }
    }
    const int k = family(&g);
    if (k == ECGVIT_KERNEL_GEMM_F32) {
        p.body = GemmBody::F32;
        p.grid = dim3(ceil_div(d->N, GEMM_F32_TILE), ceil_div(d->M, GEMM_F32_TILE), (unsigned)((int64_t)d->batch1 * d->batch2));
    } else if (k == ECGVIT_KERNEL_GEMM_NT) {
        plan_nt(p, &g);
    } else if (k == ECGVIT_KERNEL_GEMM_WGRAD) {
        plan_wgrad(p, &g);
    } else if (k == ECGVIT_KERNEL_GEMM_BF16) {
        plan_bf16(p, &g);
    }
    p.kernel = k;
    return p;
}

int run_gemm(const GemmPlan &p, const ecgvit_gemm_desc *d, void *stream) {
    if (p.kernel == ECGVIT_KERNEL_NONE) return ECGVIT_EINVAL;
    const hipStream_t s = as_stream(stream);
    ecgvit_gemm_desc g = *d;
    if (p.colsum) g.epilogue &= ~ECGVIT_EPI_COLSUM;
    int rc;
    switch (p.body) {
        case GemmBody::F32: rc = gemm_f32_launch(p, &g, s); break;
        case GemmBody::BF16: rc = gemm_bf16_launch(p, &g, s); break;
        case GemmBody::NT:
        case GemmBody::NT4W: rc = gemm_nt_launch(p, &g, s); break;
        default: rc = gemm_wgrad_launch(p, &g, s); break;
    }
    if (rc != ECGVIT_OK || !p.colsum) return rc;
    return ecgvit_colsum(d->C, d->ldc, d->colsum_out, d->workspace, d->M, d->N, d->out_dtype, stream);   // (its preconditions: colsum_args_ok)
}

}  // namespace

extern "C" int ecgvit_gemm(const ecgvit_gemm_desc *d, void *stream) { return run_gemm(plan_gemm(d, 1), d, stream); }

extern "C" int ecgvit_gemm_rowpitch(const ecgvit_gemm_desc *d, int mask_row_pitch, void *stream) {
    return run_gemm(plan_gemm(d, mask_row_pitch), d, stream);
}

extern "C" int ecgvit_gemm_kernel(const ecgvit_gemm_desc *d) { return plan_gemm(d, 1).kernel; }

extern "C" int64_t ecgvit_gemm_workspace(const ecgvit_gemm_desc *d) { return plan_gemm(d, 1).workspace; }

#ifdef ECGVIT_TOOLS
// tools build only (libecgvit_hip_tools.so): one A . B^T call with column groups of raster_g n-tiles (0 = the built-in order) on
// gemm_nt_kernel's dispatch (kernel 2) or on the four-wave body with default-policy stores (kernel 3): tools/gemm_ab.py
extern "C" int ecgvit_tools_gemm(const ecgvit_gemm_desc *d, void *stream, int kernel, int raster_g) {
    if (kernel != 2 && kernel != 3) return ecgvit_gemm(d, stream);
    GemmPlan p = plan_gemm(d, 1);
    if (p.kernel != ECGVIT_KERNEL_GEMM_NT) return ECGVIT_EINVAL;
    if (raster_g > 0) p.group = std::min(raster_g, p.tiles_n);
    if (kernel == 3) {
        if (d->dtype != ECGVIT_BF16 || d->out_dtype != ECGVIT_BF16 || d->alpha != 1.f || d->scale_a || d->scale_b ||
            !epi_in(epi_sets::FourWave{}, d->epilogue))
            return ECGVIT_EINVAL;
        p.body = GemmBody::NT4W;
        p.fl = d->epilogue;
        p.nt_stores = false;
    }
    return run_gemm(p, d, stream);
}
#endif
