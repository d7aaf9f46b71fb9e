// The GEMM front door's plan: gemm.hip decides everything about one ecgvit_gemm call (plan_gemm), the family launchers only launch it.
#pragma once
#include "common.h"
#include <type_traits>

// output tile edges and K-step of the kernel families: the planner sizes grids and split-K slabs from them
constexpr int GEMM_F32_TILE = 128, GEMM_BF16_TILE = 128, GEMM_NT_TILE = 256, GEMM_WGRAD_TILE = 256, GEMM_BK = 64;

enum class GemmBody { F32, BF16, NT, NT4W, WGRAD, WGRAD8 };   // NT4W: the four-wave A . B^T body; WGRAD8: 8-bit operands

struct GemmPlan {
    int kernel = ECGVIT_KERNEL_NONE;   // family code (ecgvit_gemm_kernel); NONE: the call returns ECGVIT_EINVAL and launches nothing
    int64_t workspace = 0;             // slab bytes of the preferred split-K factors (ecgvit_gemm_workspace)
    GemmBody body = GemmBody::F32;
    int fl = -1;                       // epilogue instantiation: a flag set with a body of its own, -1 = run-time flags
    bool nt_stores = false;            // non-temporal output stores (plain A . B^T products whose output does not fit the Infinity Cache)
    int group = 0;                     // n-tiles per column group of the A . B^T tile walk
    int tiles_m = 0, tiles_n = 0;
    int splits = 1, k_per_split = 0;   // split-K over f32 slabs in `workspace`; splits > 1: the launcher's reduce pass follows
    dim3 grid;
    bool colsum = false;               // the stand-alone column sum of the stored output follows (EPI_COLSUM off the fused bodies)
    int mask_row_pitch = 1;            // output row m draws the dropout bits of row m * mask_row_pitch
};

// The epilogue flag sets that have an A . B^T body of their own, per operand type.  The planner accepts EPI_NO_OUT and EPI_AUX8 only in
// these sets, and the launcher instantiates exactly these (epi_dispatch); any other accepted set runs the run-time-flag body (fl = -1).
template <int... F> struct EpiSets {};
namespace epi_sets {
constexpr int D = ECGVIT_EPI_DROPOUT, Q = ECGVIT_EPI_QUANT_OUT, NO = ECGVIT_EPI_NO_OUT, A8 = ECGVIT_EPI_AUX8;
constexpr int LIN = ECGVIT_EPI_BIAS | ECGVIT_EPI_RESIDUAL;                             // attn-out and FFN-down forward
constexpr int UP = ECGVIT_EPI_BIAS | ECGVIT_EPI_GELU | ECGVIT_EPI_GELU_GRAD_AUX;       // FFN-up forward
constexpr int DH = ECGVIT_EPI_MUL_AUX | ECGVIT_EPI_COLSUM;                              // FFN-down input gradient
using Bf16 = EpiSets<0, ECGVIT_EPI_BIAS, LIN, LIN | D, UP, UP | D, DH, UP | A8, UP | D | A8, DH | A8>;   // bf16 operands, bf16 output
using F32Out = EpiSets<0>;                                                                                 // bf16 operands, f32 output
using E4m3 = EpiSets<0, LIN, LIN | D, UP, UP | D, UP | Q, UP | D | Q, UP | Q | NO, UP | D | Q | NO,        // forward products
                     UP | A8, UP | D | A8, UP | Q | A8, UP | D | Q | A8, UP | Q | NO | A8, UP | D | Q | NO | A8>;
using E5m2 = EpiSets<0, DH, DH | Q, DH | Q | NO, DH | A8, DH | Q | A8, DH | Q | NO | A8>;                // input-gradient products
using FourWave = EpiSets<0, LIN, LIN | D, DH>;                                                            // the four-wave body (bf16)
}  // namespace epi_sets

template <int... F> constexpr bool epi_in(EpiSets<F...>, int fl) { return ((fl == F) || ...); }
// go(std::integral_constant<int, F>) for the set F == fl; false if fl is none of them
template <int... F, typename Go> bool epi_dispatch(EpiSets<F...>, int fl, Go &&go) {
    return ((fl == F && (go(std::integral_constant<int, F>{}), true)) || ...);
}

// the family launchers (gemm_f32.hip, gemm_bf16.hip, gemm_nt.hip, gemm_wgrad.hip): no validation, ECGVIT_OK or ECGVIT_ELAUNCH
int gemm_f32_launch(const GemmPlan &p, const ecgvit_gemm_desc *d, hipStream_t s);
int gemm_bf16_launch(const GemmPlan &p, const ecgvit_gemm_desc *d, hipStream_t s);
int gemm_nt_launch(const GemmPlan &p, const ecgvit_gemm_desc *d, hipStream_t s);
int gemm_wgrad_launch(const GemmPlan &p, const ecgvit_gemm_desc *d, hipStream_t s);
