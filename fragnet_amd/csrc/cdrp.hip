// cdrp.hip -- the cancer-drug-response model's own layers (reference model/cdrp/model.py): what sits beside the FragNet encoder in
// CDRPModel.  A translation unit of its own: nothing of the encoder or of the prediction heads reaches these kernels.
//   * the first Linear of the cell-line tower MLP(gene_dim): Y = relu(float(G) W^T + b) on the int64 gene-expression rows the reference's
//     collate_fn_cdrp produces (gene_expr.type(torch.long), cast back by .float() in MLP.forward).  gene_dim is 903 in the reference's
//     configs: K is ANY length here, rows of G and W are only element-aligned, the K tail is masked in the loads, nothing is padded.
//     Its backward has no input gradient (gene_expr is data): dW = g^T float(G), db = column sums of g.
//   * for attributions of the genes (section (b) below): the same Linear on the nodes of a straight path, and its input gradient
//     folded over the path into gradient x input / integrated gradients.
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

// ---- (b) attributions of the gene-expression input (pair_attribution.cell_line_attributions): the tower's first Linear on the points
// of a straight path, and the input gradient this layer never had, folded over the path where it is produced.
// Forward over a path: M = C S rows, row r = node j = r % S of cell line c = r / S, its input x0 + alpha[j] (float(G[c]) - x0) formed in
// the load (no float [M, K] table exists).  k_cdrp_gene_fwd's tiling, order of operations and stores: with S = 1, alpha = {1} and no
// baseline the operand is 1.f * float(G), the same bits.
template <bool TAIL, bool BASE>
__device__ __forceinline__ void gene_path_step(const long long* __restrict__ gp, const float* __restrict__ base, float al,
                                               const float* __restrict__ wp0, const float* __restrict__ wp1, int k, int K, f32x4& acc0,
                                               f32x4& acc1) {
    float a[4], b0[4], b1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool ok = !TAIL || k + q < K;
        const float x = ok ? (float)gp[k + q] : 0.f;
        if (BASE) {
            const float x0 = ok ? base[k + q] : 0.f;
            a[q] = x0 + al * (x - x0);
        } else {
            a[q] = al * x;
        }
        b0[q] = ok ? wp0[k + q] : 0.f;
        b1[q] = ok ? wp1[k + q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) { DN_MFMA(acc0, a[q], b0[q]);  DN_MFMA(acc1, a[q], b1[q]); }
}

template <bool BASE>
__global__ __launch_bounds__(256) void k_cdrp_gene_fwd_path(const long long* __restrict__ G, const float* __restrict__ base,
                                                            const float* __restrict__ alpha, const float* __restrict__ W,
                                                            const float* __restrict__ bias, float* __restrict__ Y, int M, int S, int K, int N) {
    const int l = threadIdx.x & 63, n = l & 15, g = l >> 4, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 128 + wv * 32;
    if (j0 >= N) return;
    const int r = min(i0 + n, M - 1);                    // rows / columns past the end are clamped, as in k_cdrp_gene_fwd
    const int c = r / S;
    const float al = alpha[r - c * S];
    const long long* gp = G + (size_t)c * K;
    const float* wp0 = W + (size_t)min(j0 + n, N - 1) * K;
    const float* wp1 = W + (size_t)min(j0 + 16 + n, N - 1) * K;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const int kfull = K & ~15;
#pragma unroll 2
    for (int k0 = 0; k0 < kfull; k0 += 16) gene_path_step<false, BASE>(gp, base, al, wp0, wp1, k0 + 4 * g, K, acc0, acc1);
    if (kfull < K) gene_path_step<true, BASE>(gp, base, al, wp0, wp1, kfull + 4 * g, K, acc0, acc1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = j0 + 16 * u + n;
        if (col >= N) continue;
        const float bb = bias ? bias[col] : 0.f;
        const f32x4 acc = u ? acc1 : acc0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = i0 + 4 * g + e;
            if (row < M) Y[(size_t)row * N + col] = fmaxf(acc[e] + bb, 0.f);
        }
    }
}

// Input gradient dX[M,K] = g W (the reduction over the N features), never stored: a workgroup owns `cpb` whole cell lines, rows
// [c0 S, c1 S), and 256 columns; wave w the 64 columns k in [256 bx + 64 w, + 64) as four 16 x 16 accumulators per 16-row tile.  Lane
// (n, g) reads four neighbouring features of row r0 + n of g and, per feature, sixteen lanes a contiguous run of a row of W (any K, the
// column tail masked).  Tiles are counted from the workgroup's first row, so a cell line's S rows may lie in one tile or straddle
// several; a finished tile goes through LDS and lane l then walks its sixteen rows of column j0 + l IN ORDER, adding to the running sum
// of the cell line at hand and closing it behind its last node: attr = (float(G) - x0) * (sum / S).  What a cell line's sum is does not
// depend on cpb or on where the tiles fall.
constexpr int kDxLd = 68;                                // floats per staged row: the four row groups of a store fall into distinct banks

__global__ __launch_bounds__(256) void k_cdrp_gene_dx(const float* __restrict__ g_y, const float* __restrict__ gate,
                                                      const float* __restrict__ W, const long long* __restrict__ G,
                                                      const float* __restrict__ base, float* __restrict__ attr, float* __restrict__ gavg,
                                                      int C, int S, int K, int N, int cpb) {
    __shared__ float stage[4][16 * kDxLd];
    const int l = threadIdx.x & 63, n = l & 15, g = l >> 4, wv = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 256 + wv * 64;
    const int c0 = blockIdx.y * cpb, c1 = min(c0 + cpb, C);
    const int r_begin = c0 * S, r_end = c1 * S;          // c0 < C: the grid has no empty workgroup
    float* st = stage[wv];
    const int kcol = j0 + l;                             // the column this lane folds
    const float fS = (float)S;
    float run = 0.f;
    int c = c0, jj = 0;
    const int nfull = N & ~15;
    for (int t0 = r_begin; t0 < r_end; t0 += 16) {       // the same trip count in all four waves: the barriers below are uniform
        const int r = min(t0 + n, r_end - 1);            // rows past the end are clamped: they feed sums nobody folds
        const float* gp = g_y + (size_t)r * N;
        const float* tp = gate ? gate + (size_t)r * N : nullptr;
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < N; k0 += 16) {
            const int kk = k0 + 4 * g;                   // N is a multiple of 4: a lane's four features are all there or all missing
            const bool kok = k0 < nfull || kk < N;
            float a[4], b[4][4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                a[q] = kok ? gp[kk + q] : 0.f;
                if (tp && kok && !(tp[kk + q] > 0.f)) a[q] = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int col = j0 + 16 * u + n;
                    b[q][u] = kok && col < K ? W[(size_t)(kk + q) * K + col] : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int u = 0; u < 4; ++u) DN_MFMA(acc[u], a[q], b[q][u]);
        }
        // acc[u][e] = (row t0 + 4 g + e, column j0 + 16 u + n)
        __syncthreads();                                 // the previous tile has been folded
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) st[(4 * g + e) * kDxLd + 16 * u + n] = acc[u][e];
        __syncthreads();
        const int rows = min(16, r_end - t0);
        for (int i = 0; i < rows; ++i) {                 // c, jj, rows: the same in every lane
            run += st[i * kDxLd + l];
            if (++jj == S) {
                if (kcol < K) {
                    const float mean = run / fS;
                    const size_t o = (size_t)c * K + kcol;
                    attr[o] = ((float)G[o] - (base ? base[kcol] : 0.f)) * mean;
                    if (gavg) gavg[o] = mean;
                }
                run = 0.f;
                jj = 0;
                ++c;
            }
        }
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

int fn_cdrp_gene_fwd_path_f32(const int64_t* G, const float* base, const float* alpha, const float* W, const float* bias, float* Y, int64_t C,
                              int64_t nS, int64_t K, int64_t N, fn_stream_t stream) {
    if (C < 0 || nS < 1 || nS > FN_DENSE_MAX_ROWS || C * nS > FN_DENSE_MAX_ROWS || K < 1 || K > 65536 || N < 4 || (N & 3) || N > 65536)
        return fail(FN_EINVAL, "fn_cdrp_gene_fwd_path_f32: S >= 1, K >= 1 (any), N a multiple of 4, both <= 65536, M = C S <= FN_DENSE_MAX_ROWS");
    if (C == 0) return 0;
    if (!G || !alpha || !W || !Y || ((uintptr_t)G & 7) || misaligned(3, base, alpha, W, bias, Y))
        return fail(FN_EINVAL, "fn_cdrp_gene_fwd_path_f32: null or misaligned buffer");
    const int64_t M = C * nS;
    const dim3 grid((unsigned)((M + 15) / 16), (unsigned)((N + 127) / 128));
    const long long* Gl = reinterpret_cast<const long long*>(G);
    if (base) hipLaunchKernelGGL(k_cdrp_gene_fwd_path<true>, grid, dim3(256), 0, S(stream), Gl, base, alpha, W, bias, Y, (int)M, (int)nS, (int)K, (int)N);
    else hipLaunchKernelGGL(k_cdrp_gene_fwd_path<false>, grid, dim3(256), 0, S(stream), Gl, base, alpha, W, bias, Y, (int)M, (int)nS, (int)K, (int)N);
    return launch_status("fn_cdrp_gene_fwd_path_f32");
}

int fn_cdrp_gene_dx_f32(const float* g_y, const float* y_gate, const float* W, const int64_t* G, const float* base, float* attr, float* grad_mean,
                        int64_t C, int64_t nS, int64_t K, int64_t N, fn_stream_t stream) {
    if (C < 0 || nS < 1 || nS > FN_DENSE_MAX_ROWS || C * nS > FN_DENSE_MAX_ROWS || K < 1 || K > 65536 || N < 4 || (N & 3) || N > 65536)
        return fail(FN_EINVAL, "fn_cdrp_gene_dx_f32: S >= 1, K >= 1 (any), N a multiple of 4, both <= 65536, M = C S <= FN_DENSE_MAX_ROWS");
    if (C == 0) return 0;                                 // no cell lines: nothing to write
    if (!g_y || !W || !G || !attr || ((uintptr_t)G & 7) || misaligned(3, g_y, y_gate, W, base, attr) || misaligned(3, grad_mean))
        return fail(FN_EINVAL, "fn_cdrp_gene_dx_f32: null or misaligned buffer");
    // whole cell lines per workgroup: about four 16-row tiles, so that short paths fill their tiles and long ones still spread over the CUs
    const int64_t cpb = nS >= 64 ? 1 : (64 + nS - 1) / nS;
    const dim3 grid((unsigned)((K + 255) / 256), (unsigned)((C + cpb - 1) / cpb));
    hipLaunchKernelGGL(k_cdrp_gene_dx, grid, dim3(256), 0, S(stream), g_y, y_gate, W, reinterpret_cast<const long long*>(G), base, attr, grad_mean,
                       (int)C, (int)nS, (int)K, (int)N, (int)cpb);
    return launch_status("fn_cdrp_gene_dx_f32");
}
}  // extern "C"
