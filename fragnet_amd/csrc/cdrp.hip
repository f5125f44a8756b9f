// cdrp.hip -- the cancer-drug-response model's own layers (reference model/cdrp/model.py): what sits beside the FragNet encoder in
// CDRPModel.  A translation unit of its own: nothing of the encoder or of the prediction heads reaches these kernels.
//   * the first Linear of the cell-line tower MLP(gene_dim): Y = relu(float(G) W^T + b) on the int64 gene-expression rows the reference's
//     collate_fn_cdrp produces (gene_expr.type(torch.long), cast back by .float() in MLP.forward).  gene_dim is 903 in the reference's
//     configs: K is ANY length here, rows of G and W are only element-aligned, the K tail is masked in the loads, nothing is padded.
//     Its backward has no input gradient (gene_expr is data): dW = g^T float(G), db = column sums of g.
//   * the pair head fc2(fc1(cat(drug_enc, cell_enc))) with nothing between the two Linears, 256 + 256 -> 128 -> 1, and the MSE loss on it:
//     one launch forward (the two inputs are read where they are, no cat is written), one launch backward.
// Tower layers 2-4 (1024 -> 256 -> 64 -> 256, all multiples of 4) are fn_dense_fwd_f32 / fn_dense_bwd_f32 (dense_head.inc).
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

// ---- (c) the pair head, fixed widths
constexpr int kPairIn = 256, kPairHid = 128, kPairRows = 16;

// forward: h[M,128] = drug W1[:, :256]^T + cell W1[:, 256:]^T + b1 (saved), out[M] = h w2 + b2 and, with a target, g[M] = d MSE / d out
// and one loss partial per workgroup (already divided by M: their sum in order IS the loss).  A workgroup = 16 rows, wave w the 32
// columns [32 w, + 32) of h over the 512-long reduction (the drug half, then the cell half); out from the tile in LDS: 16 lanes per row,
// 8 products each, added across the lanes in a fixed order.
__global__ __launch_bounds__(256) void k_cdrp_pair_fwd(const float* __restrict__ drug, const float* __restrict__ cell,
                                                       const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2,
                                                       const float* __restrict__ target, float* __restrict__ h, float* __restrict__ out,
                                                       float* __restrict__ g, float* __restrict__ loss_part, int M) {
    __shared__ float sh[kPairRows][kPairHid + 1];
    __shared__ float sd[kPairRows];
    const int l = threadIdx.x & 63, n = l & 15, gq = l >> 4, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.x * kPairRows, j0 = wv * 32;
    const int row = min(i0 + n, M - 1);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const float* xp = (half ? cell : drug) + (size_t)row * kPairIn + 4 * gq;
        const float* wp0 = W1 + (size_t)(j0 + n) * (2 * kPairIn) + half * kPairIn + 4 * gq;
        const float* wp1 = wp0 + (size_t)16 * (2 * kPairIn);
#pragma unroll 4
        for (int k0 = 0; k0 < kPairIn; k0 += 16) {
            const float4 a = ld4(xp + k0), p = ld4(wp0 + k0), q = ld4(wp1 + k0);
            DN_MFMA(acc0, a.x, p.x);  DN_MFMA(acc1, a.x, q.x);
            DN_MFMA(acc0, a.y, p.y);  DN_MFMA(acc1, a.y, q.y);
            DN_MFMA(acc0, a.z, p.z);  DN_MFMA(acc1, a.z, q.z);
            DN_MFMA(acc0, a.w, p.w);  DN_MFMA(acc1, a.w, q.w);
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = j0 + 16 * u + n;
        const float bb = b1[col];
        const f32x4 acc = u ? acc1 : acc0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * gq + e;
            const float v = acc[e] + bb;
            sh[r][col] = v;
            if (i0 + r < M) h[(size_t)(i0 + r) * kPairHid + col] = v;
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 4, sub = threadIdx.x & 15;
    float t = 0.f;
#pragma unroll
    for (int c = 0; c < kPairHid / 16; ++c) t = fmaf(sh[r][sub + 16 * c], w2[sub + 16 * c], t);
    t += __shfl_xor(t, 8);  t += __shfl_xor(t, 4);  t += __shfl_xor(t, 2);  t += __shfl_xor(t, 1);
    if (sub == 0) {
        float d2 = 0.f;
        if (i0 + r < M) {
            const float o = t + b2[0];
            out[i0 + r] = o;
            if (target) {
                const float d = o - target[i0 + r];
                g[i0 + r] = 2.f * d / (float)M;
                d2 = d * d;
            }
        }
        sd[r] = d2;
    }
    __syncthreads();
    if (threadIdx.x == 0 && target) {
        float s = sd[0];
        for (int q = 1; q < kPairRows; ++q) s += sd[q];
        loss_part[blockIdx.x] = s / (float)M;
    }
}

// backward, one launch.  There is nothing between the two Linears, so d loss / d h = g w2^T has rank one and every product with it folds:
//   g_x[m, k]  = g[m] v[k],     v = W1^T w2  [512]   (the cell half gated by cell > 0: the backward of the tower's last ReLU, so the
//                                                    tower's fn_dense_bwd_f32 receives its g_y ready)
//   dW1[c, k]  = w2[c] u[k],    u = [drug | cell]^T g  [512],     db1[c] = w2[c] db2,   db2 = sum_m g[m],   dW2[c] = sum_m g[m] h[m, c]
// Workgroups [0, row_blocks): 32 rows of g_drug / g_cell each (v recomputed per workgroup: 64 K products from L2);
// the next 32: 16 columns of u each for all rows (64 row lanes, added through LDS in order), then their 128 x 16 block of dW1;
// the last: dW2, db2, db1 and, with loss != null, loss[0] = sum of the forward's partials.
constexpr int kPairBwdRows = 32, kPairColBlocks = 2 * kPairIn / 16;
__global__ __launch_bounds__(256) void k_cdrp_pair_bwd(const float* __restrict__ g, const float* __restrict__ drug,
                                                       const float* __restrict__ cell, const float* __restrict__ h,
                                                       const float* __restrict__ W1, const float* __restrict__ w2,
                                                       float* __restrict__ g_drug, float* __restrict__ g_cell, float* __restrict__ dW1,
                                                       float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2,
                                                       const float* __restrict__ loss_part, int n_part, float* __restrict__ loss, int M,
                                                       int row_blocks) {
    __shared__ __attribute__((aligned(16))) float sm[1024 + 16];            // v [512] / 64 x 4 float4 partials + their 16 sums / 8 x 128 partials
    __shared__ float s1[8];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < row_blocks) {
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int k = t + 256 * rep;
            float v = 0.f;
#pragma unroll 8
            for (int c = 0; c < kPairHid; ++c) v = fmaf(w2[c], W1[(size_t)c * (2 * kPairIn) + k], v);
            sm[k] = v;
        }
        __syncthreads();
        const int m0 = b * kPairBwdRows;
        for (int e = t; e < kPairBwdRows * (2 * kPairIn / 4); e += 256) {
            const int m = m0 + e / (2 * kPairIn / 4), k = 4 * (e % (2 * kPairIn / 4));
            if (m >= M) break;
            const float gm = g[m];
            float4 o = make_float4(gm * sm[k], gm * sm[k + 1], gm * sm[k + 2], gm * sm[k + 3]);
            if (k < kPairIn) st4(g_drug + (size_t)m * kPairIn + k, o);
            else {
                const float4 cv = ld4(cell + (size_t)m * kPairIn + (k - kPairIn));
                o = make_float4(cv.x > 0.f ? o.x : 0.f, cv.y > 0.f ? o.y : 0.f, cv.z > 0.f ? o.z : 0.f, cv.w > 0.f ? o.w : 0.f);
                st4(g_cell + (size_t)m * kPairIn + (k - kPairIn), o);
            }
        }
        return;
    }
    if (b < row_blocks + kPairColBlocks) {
        const int c4 = t & 3, rl = t >> 2;
        const int col = (b - row_blocks) * 16 + 4 * c4;              // of [drug | cell]; a block's 16 columns lie in one half
        const float* x = col < kPairIn ? drug + col : cell + (col - kPairIn);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int m = rl; m < M; m += 64) fma4(acc, g[m], ld4(x + (size_t)m * kPairIn));
        st4(sm + 4 * (rl * 4 + c4), acc);
        __syncthreads();
        if (rl == 0) {
            float4 s = ld4(sm + 4 * c4);
            for (int q = 1; q < 64; ++q) { const float4 o = ld4(sm + 4 * (q * 4 + c4));  s.x += o.x;  s.y += o.y;  s.z += o.z;  s.w += o.w; }
            st4(sm + 1024 + 4 * c4, s);
        }
        __syncthreads();
        const float4 u = ld4(sm + 1024 + 4 * c4);
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int c = rl + 64 * rep;
            const float w = w2[c];
            st4(dW1 + (size_t)c * (2 * kPairIn) + col, make_float4(w * u.x, w * u.y, w * u.z, w * u.w));
        }
        return;
    }
    {                                                                 // dW2: 32 float4 columns x 8 row lanes
        const int c4 = t & 31, rl = t >> 5;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int m = rl; m < M; m += 8) fma4(acc, g[m], ld4(h + (size_t)m * kPairHid + 4 * c4));
        st4(sm + 4 * (rl * 32 + c4), acc);
        const int lane = t & 63, wv = t >> 6;
        if (wv == 0) {                                                // db2
            float s = 0.f;
            for (int m = lane; m < M; m += 64) s += g[m];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) s1[0] = s;
        }
        if (wv == 3 && loss) {                                        // the loss value: the forward left one partial per workgroup
            float s = 0.f;
            for (int i = lane; i < n_part; i += 64) s += loss_part[i];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) loss[0] = s;
        }
        __syncthreads();
        if (t < kPairHid) {
            float s = sm[t];
            for (int q = 1; q < 8; ++q) s += sm[q * kPairHid + t];
            dW2[t] = s;
            db1[t] = w2[t] * s1[0];
        }
        if (t == 0) db2[0] = s1[0];
    }
}

bool pair_widths_ok(int64_t Kd, int64_t Kc, int64_t H, int64_t C) { return Kd == kPairIn && Kc == kPairIn && H == kPairHid && C == 1; }
int pair_unsupported(const char* who) {
    (void)who;
    return fail(FN_EUNSUPPORTED, "fn_cdrp_pair_*_f32: the pair head is 256 + 256 -> 128 -> 1 (Kd = Kc = 256, H = 128, C = 1); other widths are not built");
}
bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr, const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & 15) != 0;
}
int zero_async(float* p, int64_t n, fn_stream_t stream, const char* where) {
    if (hipMemsetAsync(p, 0, (size_t)n * sizeof(float), S(stream)) != hipSuccess) return launch_status(where);
    return 0;
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

int64_t fn_cdrp_pair_loss_ws(int64_t M) { return M > 0 ? (M + kPairRows - 1) / kPairRows : 0; }

int fn_cdrp_pair_fwd_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                         const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kc, int64_t H,
                         int64_t C, fn_stream_t stream) {
    if (!pair_widths_ok(Kd, Kc, H, C)) return pair_unsupported("fn_cdrp_pair_fwd_f32");
    if (M < 0 || M > FN_DENSE_MAX_ROWS) return fail(FN_EINVAL, "fn_cdrp_pair_fwd_f32: 0 <= M <= FN_DENSE_MAX_ROWS");
    if (M == 0) return 0;
    if (!drug || !cell || !W1 || !b1 || !w2 || !b2 || !h || !out || (target && (!g || !loss_part)) || misaligned16(drug, cell, W1))
        return fail(FN_EINVAL, "fn_cdrp_pair_fwd_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_cdrp_pair_fwd, dim3((unsigned)fn_cdrp_pair_loss_ws(M)), dim3(256), 0, S(stream), drug, cell, W1, b1, w2, b2, target, h, out,
                       g, loss_part, (int)M);
    return launch_status("fn_cdrp_pair_fwd_f32");
}

int fn_cdrp_pair_bwd_f32(const float* g, const float* drug, const float* cell, const float* h, const float* W1, const float* w2, float* g_drug,
                         float* g_cell, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss,
                         int64_t M, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream) {
    if (!pair_widths_ok(Kd, Kc, H, C)) return pair_unsupported("fn_cdrp_pair_bwd_f32");
    if (M < 0 || M > FN_DENSE_MAX_ROWS || n_part < 0 || n_part > INT32_MAX) return fail(FN_EINVAL, "fn_cdrp_pair_bwd_f32: 0 <= M <= FN_DENSE_MAX_ROWS");
    if (!W1 || !w2 || !dW1 || !db1 || !dW2 || !db2 || (M > 0 && (!g || !drug || !cell || !h || !g_drug || !g_cell)) ||
        (loss && n_part > 0 && !loss_part) || misaligned16(drug, cell, h, g_drug, g_cell) || misaligned16(dW1))
        return fail(FN_EINVAL, "fn_cdrp_pair_bwd_f32: null or misaligned buffer");
    if (M == 0) {                                         // no rows: the sums are empty
        FN_TRY(zero_async(dW1, kPairHid * 2 * kPairIn, stream, "fn_cdrp_pair_bwd_f32 (no rows)"));
        FN_TRY(zero_async(db1, kPairHid, stream, "fn_cdrp_pair_bwd_f32 (no rows)"));
        FN_TRY(zero_async(dW2, kPairHid, stream, "fn_cdrp_pair_bwd_f32 (no rows)"));
        FN_TRY(zero_async(db2, 1, stream, "fn_cdrp_pair_bwd_f32 (no rows)"));
        if (loss) FN_TRY(zero_async(loss, 1, stream, "fn_cdrp_pair_bwd_f32 (no rows)"));
        return 0;
    }
    const int row_blocks = (int)((M + kPairBwdRows - 1) / kPairBwdRows);
    hipLaunchKernelGGL(k_cdrp_pair_bwd, dim3((unsigned)(row_blocks + kPairColBlocks + 1)), dim3(256), 0, S(stream), g, drug, cell, h, W1, w2, g_drug,
                       g_cell, dW1, db1, dW2, db2, loss_part, (int)n_part, loss, (int)M, row_blocks);
    return launch_status("fn_cdrp_pair_bwd_f32");
}
}  // extern "C"
