// gcn.hip -- the graph-convolution aggregate of model_version gcn2 (fragnet/model/gcn/gcn2.py:48-65): a degree-normalised neighbour
// sum over one of a level's two CSRs,
//
//     y[i] = c[i] * sum_{k in seg(i), plan order} c[nbr(k)] * x[nbr(k)]
//
// with c = deg^-1/2 on the atom graph (out-degree incl. the self loop, gcn2.py:51-54; the table is fn_gcn_coef_f32's, once per batch)
// and c == null, all ones, on the fragment graph (gcn2.py:61-65: no loops, no normalisation).  ONE kernel template for both graphs and
// both directions: the forward walks the level's by-destination CSR (rowptr_d, src_d, which holds the virtual loop items), its backward
// is the same kernel on the by-source CSR (rowptr_s, dst_s), because the weight c[s] c[t] is symmetric:
// g_x[s] = c[s] sum_{e: src = s} c[t_e] g_y[t_e].
//
// Conventions of the attention kernels (gat_fwd.inc): a 32-lane half-wave owns a 512-byte row, one float4 per lane; the items of a
// segment are summed in plan order (ascending original edge id, loop item last -- the reference's sequential scatter_add_ order), so
// results are reproducible bit for bit; no float atomics; NG source rows are in flight per half-wave before the first add; loads are
// unconditional with clamped addresses (an absent item re-reads the segment's last row, or the row itself for an empty segment, and
// is not added -- a select, not a product by 0: 0 * inf would be NaN).  A row without items is WRITTEN as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

struct GcnArgs {
    const float* x;            // [n][128] gathered rows
    const int32_t* rowptr;     // [n + 1] global positions of the chosen CSR
    const int32_t* nbr;        // [m] neighbour row at each position
    const float* coef;         // [n], nullable = all ones
    float* out;                // [n][128] raw rows, nullable
    fn_act_epilogue ep;        // ep.y nullable: relu?(dropout(.)) of the raw rows, the Philox stream of fn_dropout_act_f32
    int pos_base, n, m;
};

// NG: source rows in flight per half-wave and trip.  The level's own neighbour lists set it: an atom row has at most 5 items (4 bonds
// + the loop), the fragment rows of the ESOL-shape batches at most 6 -- not the bond graph's 12.  Longer rows (hubs) take more trips.
template <int NG>
__global__ __launch_bounds__(kBlock) void k_gcn_aggregate(GcnArgs A) {
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int n = A.n, m = A.m;
    const float* __restrict__ x = A.x;
    const uint64_t rng_base = A.ep.offset + ((A.ep.y && A.ep.p > 0.f && A.ep.offset_dev) ? *A.ep.offset_dev : 0);
    const float ik = A.ep.p < 1.f ? 1.f / (1.f - A.ep.p) : 0.f;
    int64_t g0, g1;
    block_groups(n, kRows, g0, g1);
    for (int64_t g = g0; g < g1; ++g) {                       // uniform trip count inside a block: both half-waves of a wave stay in step
        const int t = (int)g * kRows + hw;
        const bool valid = t < n;
        const int tc = valid ? t : n - 1;
        const i32x2u rp = ldp(A.rowptr + tc);
        const int beg = rp.x - A.pos_base;
        int deg = valid ? rp.y - rp.x : 0;
        if (beg < 0 || deg < 0 || beg + deg > m) deg = 0;     // (a CSR that lies outside the level: nothing is read)
        const float ct = A.coef ? A.coef[tc] : 1.f;
        const int other = __shfl_xor(deg, 32);
        const int maxdeg = deg > other ? deg : other;         // wave-uniform: the loops below never diverge
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k0 = 0; k0 < maxdeg; k0 += 32) {
            // lane l holds item k0 + l of the row: its neighbour id and coefficient (one float per gathered row)
            const bool has = k0 + lane < deg;
            int pos = beg + (has ? k0 + lane : deg - 1);
            pos = pos > m - 1 ? m - 1 : pos;
            pos = pos < 0 ? 0 : pos;                          // (maxdeg > 0 implies m > 0)
            int id = A.nbr[pos];
            id = deg > 0 && id >= 0 && id < n ? id : tc;
            const float w = A.coef ? A.coef[id] : 1.f;
            const int cnt = maxdeg - k0 < 32 ? maxdeg - k0 : 32;
            for (int q0 = 0; q0 < cnt; q0 += NG) {
                float4 r[NG];
#pragma unroll
                for (int q = 0; q < NG; ++q) {
                    const int sk = __shfl(id, (q0 + q) & 31, 32);
                    r[q] = ld4_off(x, (uint32_t)sk * (FN_D * 4) + lane * 16);
                }
#pragma unroll
                for (int q = 0; q < NG; ++q) {
                    const float wq = __shfl(w, (q0 + q) & 31, 32);
                    const bool present = q0 + q < 32 && k0 + q0 + q < deg;
                    float4 a = acc;
                    fma4(a, wq, r[q]);
                    acc.x = present ? a.x : acc.x;  acc.y = present ? a.y : acc.y;
                    acc.z = present ? a.z : acc.z;  acc.w = present ? a.w : acc.w;
                }
            }
        }
        if (A.coef) { acc.x *= ct;  acc.y *= ct;  acc.z *= ct;  acc.w *= ct; }
        if (valid) {
            const uint32_t row_off = (uint32_t)t * (FN_D * 4) + lane * 16;          // (n <= 2^23 rows: fits)
            if (A.out) st4_off(A.out, row_off, acc);
            if (A.ep.y) {        // fused act(dropout(.)): same Philox block index (element / 4) as k_dropout_act
                float4 r = acc;
                if (A.ep.p > 0.f) {
                    const uint4 rnd = philox4x32(rng_base + (uint64_t)t * 32 + lane, A.ep.seed);
                    r.x *= keep_scale(rnd.x, A.ep.p, ik);  r.y *= keep_scale(rnd.y, A.ep.p, ik);
                    r.z *= keep_scale(rnd.z, A.ep.p, ik);  r.w *= keep_scale(rnd.w, A.ep.p, ik);
                }
                if (A.ep.relu) { r.x = fmaxf(r.x, 0.f);  r.y = fmaxf(r.y, 0.f);  r.z = fmaxf(r.z, 0.f);  r.w = fmaxf(r.w, 0.f); }
                st4_off(A.ep.y, row_off, r);
            }
        }
    }
}

// c[i] = extent(i)^-1/2 over the by-source CSR (degree(source) incl. the loop item, gcn2.py:51-53), 0 where the extent is 0
__global__ __launch_bounds__(kBlock) void k_gcn_coef(const int32_t* __restrict__ rowptr_s, float* __restrict__ coef, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int d = rowptr_s[i + 1] - rowptr_s[i];
        coef[i] = d > 0 ? 1.f / sqrtf((float)d) : 0.f;
    }
}

constexpr int kGcnDepth = 6;
}  // namespace

extern "C" {

int fn_gcn_coef_f32(const fn_gat_plan* plan, float* coef, fn_stream_t stream) {
    if (!plan || plan->n < 0) return fail(FN_EINVAL, "fn_gcn_coef_f32: bad argument");
    if (plan->n == 0) return 0;
    if (!coef || !plan->rowptr_s) return fail(FN_EINVAL, "fn_gcn_coef_f32: null buffer");
    if (plan->n > (1 << 28)) return fail(FN_EUNSUPPORTED, "fn_gcn_coef_f32: level too large for 32-bit positions");
    hipLaunchKernelGGL(k_gcn_coef, dim3(flat_grid(plan->n, kGridCap)), dim3(kBlock), 0, S(stream), plan->rowptr_s, coef, (int)plan->n);
    return launch_status("fn_gcn_coef_f32");
}

int fn_gcn_aggregate_f32(const float* x, const fn_gat_plan* plan, int by_source, const float* coef, float* out,
                         const fn_act_epilogue* act, fn_stream_t stream) {
    if (!plan || plan->n < 0 || plan->m < 0) return fail(FN_EINVAL, "fn_gcn_aggregate_f32: bad argument");
    float* y = act ? act->y : nullptr;
    if (act && y && (act->p < 0.f || act->p > 1.f)) return fail(FN_EINVAL, "fn_gcn_aggregate_f32: dropout probability outside [0, 1]");
    if (plan->n == 0) return 0;                      // (no row: the buffers of an empty level may be null)
    if (!out && !y) return fail(FN_EINVAL, "fn_gcn_aggregate_f32: neither raw nor activated output requested");
    const int32_t* rowptr = by_source ? plan->rowptr_s : plan->rowptr_d;
    const int32_t* nbr = by_source ? plan->dst_s : plan->src_d;
    if (!x || !rowptr || (plan->m > 0 && !nbr)) return fail(FN_EINVAL, "fn_gcn_aggregate_f32: null buffer");
    if (misaligned(15, x, out, y) || misaligned(3, coef, rowptr, nbr)) return fail(FN_EINVAL, "fn_gcn_aggregate_f32: misaligned buffer");
    if (plan->n > (1 << 23) || plan->m > (1 << 28)) return fail(FN_EUNSUPPORTED, "fn_gcn_aggregate_f32: level too large for 32-bit byte offsets");
    GcnArgs A{};
    A.x = x;  A.rowptr = rowptr;  A.nbr = nbr;  A.coef = coef;  A.out = out;
    if (y) A.ep = *act;
    A.pos_base = by_source ? plan->pos_base_s : plan->pos_base_d;
    A.n = (int)plan->n;  A.m = (int)plan->m;
    hipLaunchKernelGGL(k_gcn_aggregate<kGcnDepth>, dim3(row_grid(plan->n, kGridCap)), dim3(kBlock), 0, S(stream), A);
    return launch_status("fn_gcn_aggregate_f32");
}

}  // extern "C"
