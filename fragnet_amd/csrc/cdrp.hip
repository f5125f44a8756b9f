// cdrp.hip -- the cancer-drug-response model's own layers (reference model/cdrp/model.py): what sits beside the FragNet encoder in
// CDRPModel.  A translation unit of its own: nothing of the encoder or of the prediction heads reaches these kernels.
//   * the first Linear of the cell-line tower MLP(gene_dim): Y = relu(float(G) W^T + b) on the int64 gene-expression rows the reference's
//     collate_fn_cdrp produces (gene_expr.type(torch.long), cast back by .float() in MLP.forward).  gene_dim is 903 in the reference's
//     configs: K is ANY length here, rows of G and W are only element-aligned, the K tail is masked in the loads, nothing is padded.
//     Its backward has no input gradient (gene_expr is data): dW = g^T float(G), db = column sums of g.
// Tower layers 2-4 (1024 -> 256 -> 64 -> 256, all multiples of 4) are fn_dense_fwd_f32 / fn_dense_bwd_f32 (dense_head.inc); the pair
// head fc2(fc1(cat(drug_enc, cell_enc))), fn_cdrp_pair_*, is the <256, true> instance of pair_head.hip.
// Arithmetic: fp32 in, fp32 accumulate, v_mfma_f32_16x16x4_f32 for the matrix products, no atomics, every sum over rows in a fixed order.
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

// ---- (a) forward.  A workgroup = 4 waves on one 16-row tile; wave w owns the 32 output columns [128 by + 32 w, + 32): two 16 x 16
// accumulators, the whole of K.  MFMA q of a 16-k step pairs k = k0 + 4 g + q of both operands in lane (n, g) = (l & 15, l >> 4), so a lane
// reads four neighbouring elements of ONE row of G and of two rows of W per step.  No LDS, no barrier: a wave without columns leaves.
template <bool TAIL>
__device__ __forceinline__ void gene_step(const long long* __restrict__ gp, const float* __restrict__ wp0, const float* __restrict__ wp1,
                                          int k, int K, f32x4& acc0, f32x4& acc1) {
    float a[4], b0[4], b1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool ok = !TAIL || k + q < K;
        a[q] = ok ? (float)gp[k + q] : 0.f;              // v_cvt_f32 of the two halves: round to nearest even, torch's .float()
        b0[q] = ok ? wp0[k + q] : 0.f;
        b1[q] = ok ? wp1[k + q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { DN_MFMA(acc0, a[q], b0[q]);  DN_MFMA(acc1, a[q], b1[q]); }
}

__global__ __launch_bounds__(256) void k_cdrp_gene_fwd(const long long* __restrict__ G, const float* __restrict__ W,
                                                       const float* __restrict__ bias, float* __restrict__ Y, int M, int K, int N) {
    const int l = threadIdx.x & 63, n = l & 15, g = l >> 4, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 128 + wv * 32;
    if (j0 >= N) return;
    // rows / columns past the end are clamped: they only feed outputs that are never stored
    const long long* gp = G + (size_t)min(i0 + n, M - 1) * K;
    const float* wp0 = W + (size_t)min(j0 + n, N - 1) * K;
    const float* wp1 = W + (size_t)min(j0 + 16 + n, N - 1) * K;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int kfull = K & ~15;
#pragma unroll 2
    for (int k0 = 0; k0 < kfull; k0 += 16) gene_step<false>(gp, wp0, wp1, k0 + 4 * g, K, acc0, acc1);
    if (kfull < K) gene_step<true>(gp, wp0, wp1, kfull + 4 * g, K, acc0, acc1);
    // acc[e] = (row i0 + 4 g + e, column j0 + 16 u + n)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = j0 + 16 * u + n;
        if (col >= N) continue;
        const float bb = bias ? bias[col] : 0.f;
        const f32x4 acc = u ? acc1 : acc0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = i0 + 4 * g + e;
            if (r < M) Y[(size_t)r * N + col] = fmaxf(acc[e] + bb, 0.f);
        }
    }
}

// ---- (a) backward: dW[N,K] = g^T float(G), db[N] = column sums of g; g = g_y, or (gate != null) g_y where gate > 0 and 0 elsewhere --
// the backward of this layer's ReLU on its saved output.  Both operands run ACROSS the reduction (the rows): lane (n, g) reads
// g_y[r0 + g][i0 + n] and G[r0 + g][j0 + 16 u + n], sixteen lanes a contiguous run, any K.  A workgroup = 4 waves on one 16-feature tile,
// wave w the 64 columns k in [256 bx + 64 w, + 64); one wave walks all M <= FN_DENSE_MAX_ROWS rows in order, four per MFMA.
__global__ __launch_bounds__(256) void k_cdrp_gene_bwd(const float* __restrict__ g_y, const float* __restrict__ gate,
                                                       const long long* __restrict__ G, float* __restrict__ dW, float* __restrict__ db,
                                                       int M, int K, int N) {
    const int l = threadIdx.x & 63, n = l & 15, g = l >> 4, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 256 + wv * 64;
    const bool do_db = db != nullptr && blockIdx.x == 0 && wv == 0;
    if (j0 >= K && !do_db) return;
    const bool iok = i0 + n < N;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float dbacc = 0.f;
#pragma unroll 2
    for (int r0 = 0; r0 < M; r0 += 4) {
        const int r = r0 + g;
        const bool rok = r < M;
        float a = 0.f, b[4];
        if (rok && iok) {
            a = g_y[(size_t)r * N + i0 + n];
            if (gate && !(gate[(size_t)r * N + i0 + n] > 0.f)) a = 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = j0 + 16 * u + n;
            b[u] = rok && k < K ? (float)G[(size_t)r * K + k] : 0.f;
        }
        dbacc += a;
#pragma unroll
        for (int u = 0; u < 4; ++u) DN_MFMA(acc[u], a, b[u]);
    }
    // acc[u][e] = (feature i0 + 4 g + e, column j0 + 16 u + n)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int k = j0 + 16 * u + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = i0 + 4 * g + e;
            if (i < N && k < K) dW[(size_t)i * K + k] = acc[u][e];
        }
    }
    if (do_db) {                                         // the four row lanes of a feature, in a fixed order
        dbacc += __shfl_xor(dbacc, 16);
        dbacc += __shfl_xor(dbacc, 32);
        if (l < 16 && iok) db[i0 + n] = dbacc;
    }
}
}  // namespace

extern "C" {

int fn_cdrp_gene_fwd_f32(const int64_t* G, const float* W, const float* bias, float* Y, int64_t M, int64_t K, int64_t N, fn_stream_t stream) {
    if (M < 0 || M > FN_DENSE_MAX_ROWS || K < 1 || K > 65536 || N < 4 || (N & 3) || N > 65536)
        return fail(FN_EINVAL, "fn_cdrp_gene_fwd_f32: K >= 1 (any), N a multiple of 4, both <= 65536, M <= FN_DENSE_MAX_ROWS");
    if (M == 0) return 0;
    if (!G || !W || !Y || ((uintptr_t)G & 7) || (((uintptr_t)W | (uintptr_t)bias | (uintptr_t)Y) & 3))
        return fail(FN_EINVAL, "fn_cdrp_gene_fwd_f32: null or misaligned buffer");
    const dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 127) / 128));
    hipLaunchKernelGGL(k_cdrp_gene_fwd, grid, dim3(256), 0, S(stream), reinterpret_cast<const long long*>(G), W, bias, Y, (int)M, (int)K, (int)N);
    return launch_status("fn_cdrp_gene_fwd_f32");
}

int fn_cdrp_gene_bwd_f32(const float* g_y, const float* y_gate, const int64_t* G, float* dW, float* db, int64_t M, int64_t K, int64_t N,
                         fn_stream_t stream) {
    if (M < 0 || M > FN_DENSE_MAX_ROWS || K < 1 || K > 65536 || N < 4 || (N & 3) || N > 65536)
        return fail(FN_EINVAL, "fn_cdrp_gene_bwd_f32: K >= 1 (any), N a multiple of 4, both <= 65536, M <= FN_DENSE_MAX_ROWS");
    if (!dW || (M > 0 && (!g_y || !G)) || ((uintptr_t)G & 7) || (((uintptr_t)g_y | (uintptr_t)y_gate | (uintptr_t)dW | (uintptr_t)db) & 3))
        return fail(FN_EINVAL, "fn_cdrp_gene_bwd_f32: null or misaligned buffer");
    if (M == 0) {                                         // no rows: the sums are empty
        FN_TRY(zero_async(dW, N * K, stream, "fn_cdrp_gene_bwd_f32 (no rows)"));
        if (db) FN_TRY(zero_async(db, N, stream, "fn_cdrp_gene_bwd_f32 (no rows)"));
        return 0;
    }
    const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((N + 15) / 16));
    hipLaunchKernelGGL(k_cdrp_gene_bwd, grid, dim3(256), 0, S(stream), g_y, y_gate, reinterpret_cast<const long long*>(G), dW, db, (int)M, (int)K,
                       (int)N);
    return launch_status("fn_cdrp_gene_bwd_f32");
}
}  // extern "C"
