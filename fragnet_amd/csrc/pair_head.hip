// pair_head.hip -- the pair head fc2(fc1(cat(drug_enc, second))) with nothing between the two Linears, 256 + K1 -> 128 -> 1, and the MSE
// loss on it: one launch forward (the two inputs are read where they are, no cat is written), one launch backward.  One kernel template
// each way, built for the two models that have such a head:
//   <256, true>    the cancer-drug-response model (reference model/cdrp/model.py:35-42), fn_cdrp_pair_*: the second input is the cell-line
//                  tower's output, the output of a ReLU, so its gradient is GATED (zero where cell <= 0: the tower's fn_dense_bwd_f32
//                  receives its g_y ready);
//   <300, false>   the drug-target-affinity model (reference model/dta/model.py:141-144), fn_dta_pair_*: the second input xt is the output
//                  of a Linear and its gradient is not gated.  300 = 18 x 16 + 12: the last MFMA step of the second half is masked, W1's
//                  rows are 556 long, and the last of the 35 column workgroups of the backward has 12 columns.
// The width and the gate are the only things that differ; both are compile-time, and no other instance is built.
// A translation unit of its own: nothing of the encoder, of the prediction heads, of cdrp.hip or of dta.hip reaches these kernels.
// Arithmetic: fp32 in, fp32 accumulate, v_mfma_f32_16x16x4_f32 for the matrix products, no atomics, every sum over rows in a fixed order.
// Orders of additions: v = W1^T w2 and the last workgroup's sums (dW2, db2, the loss) are pair_bodies.inc's, shared with pair_factored.hip;
// the tile-row dot with w2 and the end of a dW1 column block are written here and, the same statements, in pair_factored.hip (why:
// pair_bodies.inc); this unit's own are the forward's two-half accumulation and loss partial and the backward's sums over rows.
#include <stdint.h>
#include <stdio.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

#include "pair_bodies.inc"
constexpr int kPairRows = 16, kPairBwdRows = 32;

// forward: h[M,128] = drug W1[:, :256]^T + x1 W1[:, 256:]^T + b1 (saved), out[M] = h w2 + b2 and, with a target, g[M] = d MSE / d out
// and one loss partial per workgroup (already divided by M: their sum in order IS the loss).  A workgroup = 16 rows, wave w the 32
// columns [32 w, + 32) of h over the (256 + K1)-long reduction: 16 full steps of the drug half, then the full steps of the second half
// and, where K1 is no multiple of 16, one of which the quarters behind K1 are masked; out from the tile in LDS: 16 lanes per row,
// 8 products each, added across the lanes in a fixed order.
// real_rows (nullable; fn_*_pair_fwd_rows_f32): the int32 word a static-shape step's staging launch writes (FN_STAGE_COUNT), n = *real_rows
// clamped to [0, M].  The mean is then over the first n rows: g = 2 (out - y) / n and the partials are divided by n there, g = 0 exactly
// and no share of the loss behind them (their out is still written); n = 0: every g and every partial is 0, nothing is divided.  The
// backward needs no count: a zero g makes every term of a padding row an exact zero, in the same place of the same sums.
template <int K1>
__global__ __launch_bounds__(256) void k_pair_fwd(const float* __restrict__ drug, const float* __restrict__ x1, const float* __restrict__ W1,
                                                  const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                  const float* __restrict__ target, float* __restrict__ h, float* __restrict__ out,
                                                  float* __restrict__ g, float* __restrict__ loss_part, int M,
                                                  const int* __restrict__ real_rows) {
    constexpr int kInT = kIn0 + K1, kfull = K1 & ~15, kUnroll1 = kfull < K1 ? 2 : 4;
    __shared__ float sh[kPairRows][kHid + 1];
    __shared__ float sd[kPairRows];
    const int l = threadIdx.x & 63, n = l & 15, gq = l >> 4, wv = threadIdx.x >> 6;
    const int i0 = blockIdx.x * kPairRows, j0 = wv * 32;
    const int row = min(i0 + n, M - 1);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    {
        const float* xp = drug + (size_t)row * kIn0 + 4 * gq;
        const float* wp0 = W1 + (size_t)(j0 + n) * kInT + 4 * gq;
        const float* wp1 = wp0 + (size_t)16 * kInT;
#pragma unroll 4
        for (int k0 = 0; k0 < kIn0; k0 += 16) pair_step(xp + k0, wp0 + k0, wp1 + k0, true, acc0, acc1);
    }
    {
        const float* xp = x1 + (size_t)row * K1 + 4 * gq;
        const float* wp0 = W1 + (size_t)(j0 + n) * kInT + kIn0 + 4 * gq;
        const float* wp1 = wp0 + (size_t)16 * kInT;
#pragma unroll kUnroll1
        for (int k0 = 0; k0 < kfull; k0 += 16) pair_step(xp + k0, wp0 + k0, wp1 + k0, true, acc0, acc1);
        if constexpr (kfull < K1) pair_step(xp + kfull, wp0 + kfull, wp1 + kfull, kfull + 4 * gq < K1, acc0, acc1);
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
            if (i0 + r < M) h[(size_t)(i0 + r) * kHid + col] = v;
        }
    }
    __syncthreads();
    const int r = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const int nr = real_rows ? min(max(*real_rows, 0), M) : M;      // rows the loss is a mean over: all of them without a count
    float t = 0.f;                                                   // the tile-row dot: the same statements, the same order as k_pairf_fwd's
#pragma unroll
    for (int c = 0; c < kHid / 16; ++c) t = fmaf(sh[r][sub + 16 * c], w2[sub + 16 * c], t);
    t += __shfl_xor(t, 8);  t += __shfl_xor(t, 4);  t += __shfl_xor(t, 2);  t += __shfl_xor(t, 1);
    if (sub == 0) {
        float d2 = 0.f;
        if (i0 + r < M) {
            const float o = t + b2[0];
            out[i0 + r] = o;
            if (target) {
                if (i0 + r < nr) {
                    const float d = o - target[i0 + r];
                    g[i0 + r] = 2.f * d / (float)nr;
                    d2 = d * d;
                } else
                    g[i0 + r] = 0.f;                                 // a padding row: no gradient, no share of the loss
            }
        }
        sd[r] = d2;
    }
    __syncthreads();
    if (threadIdx.x == 0 && target) {
        float s = sd[0];
        for (int q = 1; q < kPairRows; ++q) s += sd[q];
        loss_part[blockIdx.x] = nr > 0 ? s / (float)nr : 0.f;
    }
}

// backward, one launch.  There is nothing between the two Linears, so d loss / d h = g w2^T has rank one and every product with it folds:
//   g_x[m, k]  = g[m] v[k],     v = W1^T w2  [256 + K1]   (GATE: the second half zeroed where x1 <= 0, the backward of the ReLU that
//                                                         produced x1; else both halves as they are)
//   dW1[c, k]  = w2[c] u[k],    u = [drug | x1]^T g  [256 + K1],  db1[c] = w2[c] db2,   db2 = sum_m g[m],   dW2[c] = sum_m g[m] h[m, c]
// Workgroups [0, row_blocks): 32 rows of g_drug / g_x1 each (v recomputed per workgroup: 64 K products from L2);
// the next ceil((256 + K1) / 16): 16 columns of u each (K1 = 300: the last one 12) for all rows (64 row lanes, added through LDS in
// order), then their 128 x 16 block of dW1; the last: dW2, db2, db1 and, with loss != null, loss[0] = sum of the forward's partials.
template <int K1, bool GATE>
__global__ __launch_bounds__(256) void k_pair_bwd(const float* __restrict__ g, const float* __restrict__ drug, const float* __restrict__ x1,
                                                  const float* __restrict__ h, const float* __restrict__ W1, const float* __restrict__ w2,
                                                  float* __restrict__ g_drug, float* __restrict__ g_x1, float* __restrict__ dW1,
                                                  float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2,
                                                  const float* __restrict__ loss_part, int n_part, float* __restrict__ loss, int M,
                                                  int row_blocks) {
    constexpr int kInT = kIn0 + K1;
    static_assert(K1 % 4 == 0 && kInT <= 1024, "float4 columns; v fits the LDS array");
    __shared__ __attribute__((aligned(16))) float sm[1024 + 16];            // v [kInT] / 64 x 4 float4 partials + their 16 sums / 8 x 128 partials
    __shared__ float s1[8];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < row_blocks) {
        if constexpr (kInT % 256 == 0) {                              // every thread the same number of columns: no bound to test
#pragma unroll
            for (int rep = 0; rep < kInT / 256; ++rep) sm[t + 256 * rep] = pair_v<kInT>(w2, W1, t + 256 * rep);
        } else
            for (int k = t; k < kInT; k += 256) sm[k] = pair_v<kInT>(w2, W1, k);
        __syncthreads();
        const int m0 = b * kPairBwdRows;
        for (int e = t; e < kPairBwdRows * (kInT / 4); e += 256) {
            const int m = m0 + e / (kInT / 4), k = 4 * (e % (kInT / 4));
            if (m >= M) break;
            const float gm = g[m];
            float4 o = make_float4(gm * sm[k], gm * sm[k + 1], gm * sm[k + 2], gm * sm[k + 3]);
            if (k < kIn0) st4(g_drug + (size_t)m * kIn0 + k, o);
            else {
                if constexpr (GATE) o = relu_gate4(o, ld4(x1 + (size_t)m * K1 + (k - kIn0)));
                st4(g_x1 + (size_t)m * K1 + (k - kIn0), o);
            }
        }
        return;
    }
    if (b < row_blocks + kPairColBlocks<K1>) {
        const int c4 = t & 3, rl = t >> 2;
        const int col = (b - row_blocks) * 16 + 4 * c4;              // of [drug | x1]; 256 = 16 blocks: a block's columns lie in one half
        const bool ok = kInT % 16 == 0 || col < kInT;
        const float* x = col < kIn0 ? drug + col : x1 + (col - kIn0);
        const int ldx = col < kIn0 ? kIn0 : K1;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok)
            for (int m = rl; m < M; m += 64) fma4(acc, g[m], ld4(x + (size_t)m * ldx));
        st4(sm + 4 * (rl * 4 + c4), acc);                            // from here: the same statements, the same order as k_pairf_bwd's
        __syncthreads();
        if (rl == 0) {
            float4 s = ld4(sm + 4 * c4);
            for (int q = 1; q < 64; ++q) { const float4 o = ld4(sm + 4 * (q * 4 + c4));  s.x += o.x;  s.y += o.y;  s.z += o.z;  s.w += o.w; }
            st4(sm + 1024 + 4 * c4, s);
        }
        __syncthreads();
        if (!ok) return;
        const float4 u = ld4(sm + 1024 + 4 * c4);
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {
            const int c = rl + 64 * rep;
            const float w = w2[c];
            st4(dW1 + (size_t)c * kInT + col, make_float4(w * u.x, w * u.y, w * u.z, w * u.w));
        }
        return;
    }
    {                                                                 // dW2: 32 float4 columns x 8 row lanes
        const int c4 = t & 31, rl = t >> 5;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int m = rl; m < M; m += 8) fma4(acc, g[m], ld4(h + (size_t)m * kHid + 4 * c4));
        pair_last_tail(acc, sm, s1, g, M, w2, loss_part, n_part, loss, db1, dW2, db2, [](float s, int, float) { return s; });
    }
}

// ---- host side (fail_at, check_widths, zero_param_grads: pair_bodies.inc)
int64_t pair_loss_ws(int64_t M) { return M > 0 ? (M + kPairRows - 1) / kPairRows : 0; }

template <int K1>
int pair_fwd(const char* who, const float* drug, const float* x1, const float* W1, const float* b1, const float* w2, const float* b2,
             const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t K, int64_t H, int64_t C,
             const int32_t* real_rows, fn_stream_t stream) {
    FN_TRY(check_widths<K1>("pair_*_f32", Kd, K, H, C));
    if (M < 0 || M > FN_DENSE_MAX_ROWS) return fail_at(FN_EINVAL, who, "0 <= M <= FN_DENSE_MAX_ROWS");
    if (M == 0) return 0;
    if (!drug || !x1 || !W1 || !b1 || !w2 || !b2 || !h || !out || (target && (!g || !loss_part)) || misaligned(15, drug, x1, W1))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    if (real_rows && (!target || ((uintptr_t)real_rows & 3))) return fail_at(FN_EINVAL, who, "a real-row count goes with a target (and is an aligned int32)");
    hipLaunchKernelGGL(k_pair_fwd<K1>, dim3((unsigned)pair_loss_ws(M)), dim3(256), 0, S(stream), drug, x1, W1, b1, w2, b2, target, h, out, g,
                       loss_part, (int)M, real_rows);
    return launch_status(who);
}

template <int K1, bool GATE>
int pair_bwd(const char* who, const float* g, const float* drug, const float* x1, const float* h, const float* W1, const float* w2,
             float* g_drug, float* g_x1, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss,
             int64_t M, int64_t Kd, int64_t K, int64_t H, int64_t C, fn_stream_t stream) {
    FN_TRY(check_widths<K1>("pair_*_f32", Kd, K, H, C));
    if (M < 0 || M > FN_DENSE_MAX_ROWS || n_part < 0 || n_part > INT32_MAX) return fail_at(FN_EINVAL, who, "0 <= M <= FN_DENSE_MAX_ROWS");
    if (!W1 || !w2 || !dW1 || !db1 || !dW2 || !db2 || (M > 0 && (!g || !drug || !x1 || !h || !g_drug || !g_x1)) ||
        (loss && n_part > 0 && !loss_part) || misaligned(15, drug, x1, h, g_drug, g_x1) || misaligned(15, dW1))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    if (M == 0) {                                         // no rows: the sums are empty
        char where[64];
        snprintf(where, sizeof(where), "%s (no rows)", who);
        return zero_param_grads<K1>(dW1, db1, dW2, db2, loss, stream, where);
    }
    const int row_blocks = (int)((M + kPairBwdRows - 1) / kPairBwdRows);
    hipLaunchKernelGGL((k_pair_bwd<K1, GATE>), dim3((unsigned)(row_blocks + kPairColBlocks<K1> + 1)), dim3(256), 0, S(stream), g, drug, x1, h, W1, w2,
                       g_drug, g_x1, dW1, db1, dW2, db2, loss_part, (int)n_part, loss, (int)M, row_blocks);
    return launch_status(who);
}
}  // namespace

extern "C" {

int64_t fn_cdrp_pair_loss_ws(int64_t M) { return pair_loss_ws(M); }
int64_t fn_dta_pair_loss_ws(int64_t M) { return pair_loss_ws(M); }

int fn_cdrp_pair_fwd_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                         const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kc, int64_t H,
                         int64_t C, fn_stream_t stream) {
    return pair_fwd<256>("fn_cdrp_pair_fwd_f32", drug, cell, W1, b1, w2, b2, target, h, out, g, loss_part, M, Kd, Kc, H, C, nullptr, stream);
}
int fn_cdrp_pair_fwd_rows_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                              const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kc, int64_t H,
                              int64_t C, const int32_t* real_rows, fn_stream_t stream) {
    return pair_fwd<256>("fn_cdrp_pair_fwd_rows_f32", drug, cell, W1, b1, w2, b2, target, h, out, g, loss_part, M, Kd, Kc, H, C, real_rows, stream);
}
int fn_dta_pair_fwd_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                        const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kx, int64_t H,
                        int64_t C, fn_stream_t stream) {
    return pair_fwd<300>("fn_dta_pair_fwd_f32", drug, xt, W1, b1, w2, b2, target, h, out, g, loss_part, M, Kd, Kx, H, C, nullptr, stream);
}
int fn_dta_pair_fwd_rows_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                             const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kx, int64_t H,
                             int64_t C, const int32_t* real_rows, fn_stream_t stream) {
    return pair_fwd<300>("fn_dta_pair_fwd_rows_f32", drug, xt, W1, b1, w2, b2, target, h, out, g, loss_part, M, Kd, Kx, H, C, real_rows, stream);
}

int fn_cdrp_pair_bwd_f32(const float* g, const float* drug, const float* cell, const float* h, const float* W1, const float* w2, float* g_drug,
                         float* g_cell, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss,
                         int64_t M, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream) {
    return pair_bwd<256, true>("fn_cdrp_pair_bwd_f32", g, drug, cell, h, W1, w2, g_drug, g_cell, dW1, db1, dW2, db2, loss_part, n_part, loss, M, Kd,
                               Kc, H, C, stream);
}
int fn_dta_pair_bwd_f32(const float* g, const float* drug, const float* xt, const float* h, const float* W1, const float* w2, float* g_drug,
                        float* g_xt, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss,
                        int64_t M, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream) {
    return pair_bwd<300, false>("fn_dta_pair_bwd_f32", g, drug, xt, h, W1, w2, g_drug, g_xt, dW1, db1, dW2, db2, loss_part, n_part, loss, M, Kd, Kx,
                                H, C, stream);
}
}  // extern "C"
