// gat_fwd.hip -- the attention forward of one level / of two independent levels (k_gat_fwd, k_gat_fwd_pair, k_gat_fwd_rd) and their
// host side (argument validation, launch geometry, fn_gat_fwd_f32).  A translation unit of its own since round 5: the family's
// instantiations (heads x edge classes x second output x fused row dots) were 60 % of the library's compile time.
#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;
using fni::tune;
using fni::bad_edge_term;
#include "gat_fwd.inc"

// (O2 instances -- the training forward of the one-pass backward, gat_bwd_one.inc -- ask for four waves per SIMD explicitly: their
// second accumulator would otherwise tip the allocation over 128 registers)
template <int H, int KL, int O2 = 0>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd(GatFwdArgs A) {
    __shared__ float sWf[8][kWfLd];
    gat_fwd_body<H, KL, false, O2>(A, sWf, (int)blockIdx.x, (int)gridDim.x);
}
// two independent levels in one launch (bond graph + fragment-bond graph: neither reads the other's output)
template <int H, int KLA, int KLB, bool RDA = false, int O2 = 0>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd_pair(GatFwdArgs A, GatFwdArgs B) {
    __shared__ float sWf[8][kWfLd];
    if ((int)blockIdx.x < A.nblk) gat_fwd_body<H, KLA, RDA, O2>(A, sWf, (int)blockIdx.x, A.nblk);
    else gat_fwd_body<H, KLB, false, O2>(B, sWf, (int)blockIdx.x - A.nblk, B.nblk);
}
template <int H, int O2 = 0>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd_rd(GatFwdArgs A) {          // single bond-graph level with the row-dots epilogue
    __shared__ float sWf[8][kWfLd];
    gat_fwd_body<H, 1, true, O2>(A, sWf, (int)blockIdx.x, (int)gridDim.x);
}

// ---- kind 4 (gat_fwd.inc): the masked evaluation forward of fn_encoder_forward_masked.  Kernels of their own -- the mask pointers are
// kernel arguments beside the level's block, so that kinds 0-3 and their argument blocks stay what they were.  A null pointer is a level
// without a mask of its own in a masked pass.
template <int H, int KL>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd_m(GatFwdArgs A, const uint8_t* mk) {
    __shared__ float sWf[8][kWfLd];
    gat_fwd_body<H, KL, false, 4>(A, sWf, (int)blockIdx.x, (int)gridDim.x, mk);
}
template <int H, int KLA, int KLB, bool RDA>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd_pair_m(GatFwdArgs A, GatFwdArgs B, const uint8_t* mka, const uint8_t* mkb) {
    __shared__ float sWf[8][kWfLd];
    if ((int)blockIdx.x < A.nblk) gat_fwd_body<H, KLA, RDA, 4>(A, sWf, (int)blockIdx.x, A.nblk, mka);
    else gat_fwd_body<H, KLB, false, 4>(B, sWf, (int)blockIdx.x - A.nblk, B.nblk, mkb);
}
template <int H>
__global__ __launch_bounds__(kBlock, 4) void k_gat_fwd_rd_m(GatFwdArgs A, const uint8_t* mk) {
    __shared__ float sWf[8][kWfLd];
    gat_fwd_body<H, 1, true, 4>(A, sWf, (int)blockIdx.x, (int)gridDim.x, mk);
}

}  // namespace

namespace fni {
int prep_gat_fwd(const float* h, const float* s_dst, const float* s_src, const float* att, int att_w,
                        const fn_edge_term* et, const fn_gat_plan* plan, float neg_slope, float* out, float* p_sorted,
                        float* probs_orig, const fn_act_epilogue* act, int heads, GatFwdArgs* A, float* out2,
                        float* sigma) {
    if (!h || !s_dst || !s_src || !att || !plan || bad_edge_term(et, plan->m)) return fail(FN_EINVAL, "fn_gat_fwd_f32: bad argument");
    if (!out && !(act && act->y)) return fail(FN_EINVAL, "fn_gat_fwd_f32: no output buffer");
    if (act && (act->p < 0.f || act->p > 1.f)) return fail(FN_EINVAL, "fn_gat_fwd_f32: dropout probability");
    if (plan->m > 0 && !p_sorted) return fail(FN_EINVAL, "fn_gat_fwd_f32: null p_sorted");
    if (et->mode == 0 && plan->m > 0 && !et->s_sorted) return fail(FN_EINVAL, "fn_gat_fwd_f32: null s_sorted");
    if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return fail(FN_EUNSUPPORTED, "heads must be 1, 2, 4 or 8 (128 = heads * head_dim)");
    *A = GatFwdArgs{h, s_dst, s_src, att, att_w, *et, *plan, neg_slope, out, p_sorted, probs_orig,
                    act ? *act : fn_act_epilogue{nullptr, 0.f, 0, 0, 0, nullptr}, 1, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0, nullptr, tune(FN_TUNE_ONE_TIER6) != 0 ? 1 : 0};
    if ((out2 == nullptr) != (sigma == nullptr)) return fail(FN_EINVAL, "fn_gat_fwd_f32: out2 and sigma come together");
    A->out2 = out2;  A->sigma = sigma;
    if (plan->n == 0) return 0;
    if (!(neg_slope >= 0.f && neg_slope <= 1.f)) return fail(FN_EUNSUPPORTED, "fn_gat_fwd_f32: LeakyReLU slope must be in [0, 1]");
    if (plan->n > (1 << 23) || plan->m * heads > (1 << 29))
        return fail(FN_EUNSUPPORTED, "fn_gat_fwd_f32: level too large for 32-bit byte offsets (n <= 2^23 rows, m*heads <= 2^29)");
    // persistent half-waves: as many as fit on the chip at once, each pipelining R rows
    const int64_t groups = (plan->n + kRows - 1) / kRows;
    // with the dropout epilogue (training) fewer, longer-lived half-waves win (5 rows each at B = 512: 27.7 -> 22.4 us for the
    // bond + fragment-bond launch); the plain forward (inference) wants the chip full of them
    const bool training = act && act->y && act->p > 0.f;
    int64_t resident = (int64_t)tune(training ? FN_TUNE_FWD_BLOCKS : FN_TUNE_FWD_BLOCKS_EVAL);
    // ... but not arbitrarily long-lived: a large level (2048+ molecules per batch) made every half-wave of the plain forward walk
    // 12-46 rows and the launch wait for its slowest workgroups -- it gets FN_TUNE_FWD_BLOCKS_EVAL_LARGE workgroups instead (round 5)
    const int64_t large = (int64_t)tune(FN_TUNE_FWD_BLOCKS_EVAL_LARGE);
    if (!training && large > resident && groups > 4 * resident) resident = large;
    A->rows_per_hw = (int)((groups + resident - 1) / resident);
    A->nblk = (int)((plan->n + (int64_t)kRows * A->rows_per_hw - 1) / ((int64_t)kRows * A->rows_per_hw));
    return 0;
}

// Which instance a launch takes: the kind from fwd_kind / fwd_kind_pair (fn_internal.h), the edge class(es) of the level(s), whether the
// row dots ride in the epilogue.  Kernels exist for: kinds 2, 3, 4 -- four heads; row dots -- edge class 1; two levels -- classes (1, 1)
// and (1, FN_MAX_EDGE_K).
int launch_gat_fwd(const GatFwdArgs& A, int heads, hipStream_t st, const FwdMask* mk) {
    if (A.nblk == 0) return 0;
    const int kl = edge_class(&A.et), kind = fwd_kind(A, heads, mk != nullptr);
    if (kind == kFwdNoKind) return fail(FN_EUNSUPPORTED, "attention forward: a masked level is a four-head evaluation level without second output");
    if (A.rd_out && kl != 1) return fail(FN_EUNSUPPORTED, "attention forward: the row-dots epilogue exists for the single-attribute (bond graph) level");
    const dim3 grid(A.nblk), block(kBlock);
    if (kind == 4) {
        if (A.rd_out) hipLaunchKernelGGL((k_gat_fwd_rd_m<4>), grid, block, 0, st, A, mk->rows);
        else with_edge_class(kl, [&](auto KL) { hipLaunchKernelGGL((k_gat_fwd_m<4, FN_CV(KL)>), grid, block, 0, st, A, mk->rows); });
        return launch_status("fn_gat_fwd_f32 (masked rows)");
    }
    if (A.rd_out) {
        // k_gat_fwd_rd exists for the plain kinds 0 and 1 only (and as kind 4, above): a level that qualifies for kind 3 / 2 runs as 0 / 1 here
        if (!with_const<1, 2, 4, 8>(heads, [&](auto H) { with_const<0, 1>(fwd_kind_plain(kind), [&](auto O2) {
                hipLaunchKernelGGL((k_gat_fwd_rd<FN_CV(H), FN_CV(O2)>), grid, block, 0, st, A);
            }); })) return bad_heads();
        return launch_status("fn_gat_fwd_f32 (+ row dots)");
    }
    FN_TRY(with_heads_kind(heads, kind, [&](auto H, auto O2) {
        with_edge_class(kl, [&](auto KL) { hipLaunchKernelGGL((k_gat_fwd<FN_CV(H), FN_CV(KL), FN_CV(O2)>), grid, block, 0, st, A); });
    }));
    return launch_status("fn_gat_fwd_f32");
}
// two levels, one launch, when their edge classes are (1, FN_MAX_EDGE_K) or (1, 1) and they have a kind in common; two launches otherwise
int launch_gat_fwd_pair(const GatFwdArgs& A, const GatFwdArgs& B, int heads, hipStream_t st, const FwdMask* mka, const FwdMask* mkb) {
    const int kb = edge_class(&B.et), kind = fwd_kind_pair(A, B, heads, mka, mkb), rd = A.rd_out != nullptr;
    if (!fwd_pair_classes(A, B) || (kind == kFwdNoKind && !mka && !mkb)) {
        if (int rc = launch_gat_fwd(A, heads, st, mka)) return rc;
        return launch_gat_fwd(B, heads, st, mkb);
    }
    if (kind == kFwdNoKind) return fail(FN_EUNSUPPORTED, "attention forward (two levels): masked levels are four-head evaluation levels without second output");
    const dim3 grid(A.nblk + B.nblk), block(kBlock);
    if (kind == 4) {
        with_const<1, FN_MAX_EDGE_K>(kb, [&](auto KB) { with_const<0, 1>(rd, [&](auto RD) {
            hipLaunchKernelGGL((k_gat_fwd_pair_m<4, 1, FN_CV(KB), FN_CV(RD) != 0>), grid, block, 0, st, A, B, mka->rows, mkb->rows);
        }); });
        return launch_status("attention forward (two levels, masked rows)");
    }
    FN_TRY(with_heads_kind(heads, kind, [&](auto H, auto O2) { with_const<1, FN_MAX_EDGE_K>(kb, [&](auto KB) { with_const<0, 1>(rd, [&](auto RD) {
        hipLaunchKernelGGL((k_gat_fwd_pair<FN_CV(H), 1, FN_CV(KB), FN_CV(RD) != 0, FN_CV(O2)>), grid, block, 0, st, A, B);
    }); }); }));
    return launch_status("attention forward (two levels)");
}

}  // namespace fni

using fni::prep_gat_fwd;
using fni::launch_gat_fwd;
using fni::GatFwdArgs;
extern "C" {
int fn_gat_fwd_f32(const float* h, const float* s_dst, const float* s_src, const float* att, int att_w,
                   const fn_edge_term* et, const fn_gat_plan* plan, float neg_slope, float* out, float* p_sorted,
                   float* probs_orig, float* out2, float* sigma, int p_edge_major, const fn_act_epilogue* act, int heads,
                   fn_stream_t stream) {
    GatFwdArgs A;
    if (int rc = prep_gat_fwd(h, s_dst, s_src, att, att_w, et, plan, neg_slope, out, p_sorted, probs_orig, act, heads, &A, out2, sigma)) return rc;
    A.p_edge_major = p_edge_major ? 1 : 0;
    return launch_gat_fwd(A, heads, S(stream));
}
}  // extern "C"
