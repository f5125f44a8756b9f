// head.hip -- the prediction head (reference model/gat/gat2.py:569-751, FTHead1-5: act(dropout(Linear(x))) stacks on [molecules, width]
// and a last Linear of n_classes columns): the dense products on the fp32 matrix cores with their element-wise work fused in
// (dense_head.inc), the activation kinds other than the ReLU fast path (head_act.inc), the last Linear with its backward and its fused
// loss (k_small_linear*), the gated column sums, and their fn_gate_colsum*, fn_small_linear*, fn_dense_* and fn_head_act_* entry points.
// A translation unit of its own: no launch of the encoder reaches these kernels, and they carry the library's widest instance fan-out
// (nine activation instances of each dense kernel).
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;
using fni::tune;

#include "zero2.inc"

// =====================================================================================
// Prediction-head small ops (gat2.py:631-637, 745-751: Linear -> dropout -> ReLU stacks on [molecules, width]).
// The dense products stay library GEMMs; these are the launches around them.
// =====================================================================================
// g_x = (y > 0) ? g_y * scale : 0  and  colsum[c] = sum_rows g_x[:, c]   (bias gradient of the Linear below)
// y = relu(dropout(.)) is positive only where the element was kept and passed the ReLU, so no Philox replay.
// One block owns a strip of 32 columns for ALL rows: the column sums are deterministic and need no second pass.
__global__ __launch_bounds__(256) void k_gate_colsum(const float* __restrict__ g_y, const float* __restrict__ y,
                                                     float* __restrict__ g_x, float* __restrict__ sums, int64_t rows,
                                                     int cols, float scale, int64_t rows_per_chunk) {
    // blockIdx.y = row chunk (tall inputs: the pretrain towers run on every edge / atom); its column sums go to
    // sums[chunk][cols] and k_sum_chunks adds the chunks in order.  One chunk: sums is the result itself.
    __shared__ float4 sm[32][8];
    const int c4 = threadIdx.x & 7, rl = threadIdx.x >> 3;           // 8 float4 columns x 32 row lanes
    const int col = blockIdx.x * 32 + c4 * 4;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r_end = r_begin + rows_per_chunk < rows ? r_begin + rows_per_chunk : rows;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col < cols) {
        int64_t r = r_begin + rl;
        for (; r + 96 < r_end; r += 128) {                          // four rows in flight per thread
            float4 g[4], v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { g[q] = ld4(g_y + (r + 32 * q) * cols + col); v[q] = ld4(y + (r + 32 * q) * cols + col); }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 o = make_float4(v[q].x > 0.f ? g[q].x * scale : 0.f, v[q].y > 0.f ? g[q].y * scale : 0.f,
                                             v[q].z > 0.f ? g[q].z * scale : 0.f, v[q].w > 0.f ? g[q].w * scale : 0.f);
                st4(g_x + (r + 32 * q) * cols + col, o);
                acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
            }
        }
        for (; r < r_end; r += 32) {
            const float4 g = ld4(g_y + r * cols + col), v = ld4(y + r * cols + col);
            const float4 o = make_float4(v.x > 0.f ? g.x * scale : 0.f, v.y > 0.f ? g.y * scale : 0.f,
                                         v.z > 0.f ? g.z * scale : 0.f, v.w > 0.f ? g.w * scale : 0.f);
            st4(g_x + r * cols + col, o);
            acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
    }
    sm[rl][c4] = acc;
    __syncthreads();
    if (rl == 0 && col < cols) {
        float4 t = sm[0][c4];
        for (int q = 1; q < 32; ++q) { const float4 u = sm[q][c4]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
        st4(sums + (size_t)blockIdx.y * cols + col, t);
    }
}
// out[c] = sum over chunks of part[chunk][c] in a fixed order: 16 chunk lanes each add every 16th chunk, then the 16
// lane sums are added in lane order (a serial walk over ~110 dependent loads took 25 us)
__global__ __launch_bounds__(256) void k_sum_chunks(const float* __restrict__ part, int chunks, int64_t width, float* __restrict__ out) {
    __shared__ float sm[16][17];
    const int cl = threadIdx.x & 15, ql = threadIdx.x >> 4;
    const int64_t c = (int64_t)blockIdx.x * 16 + cl;
    float t = 0.f;
    if (c < width)
        for (int q = ql; q < chunks; q += 16) t += part[(size_t)q * width + c];
    sm[ql][cl] = t;
    __syncthreads();
    if (ql == 0 && c < width) {
        float v = sm[0][cl];
        for (int q = 1; q < 16; ++q) v += sm[q][cl];
        out[c] = v;
    }
}

// y[m, c] = <x[m, :], w[c, :]> + b[c] for a handful of outputs (the last Linear of a head: n_classes columns).
// One wave per row; the row stays in registers while the C weight rows stream from L1.
__global__ __launch_bounds__(256) void k_small_linear(const float* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ b, float* __restrict__ y, int64_t M, int K, int C,
                                                      int64_t M_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) {                                                  // padding rows of a static-shape batch: defined, 0
        if (row < M_out && lane < C) y[row * C + lane] = 0.f;
        return;
    }
    const int k4 = K / 4;                                            // K % 4 == 0
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        for (int j = lane; j < k4; j += 64) acc += dot4(ld4(x + row * K + 4 * j), ld4(w + (size_t)c * K + 4 * j));
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) y[row * C + c] = acc + (b ? b[c] : 0.f);
    }
}

#include "head_act.inc"

// backward of the above in one launch: g_x[m, k] = sum_c g[m, c] w[c, k];  dW[c, k] = sum_m g[m, c] x[m, k];
// db[c] = sum_m g[m, c].  A block owns 16 columns k for all rows (deterministic sums, 64 rows in flight);
// CM >= C bounds the registers.  HACT: g_x goes through the activation kind `below` (head_act.inc) instead of the ReLU gate.
template <int CM, bool HACT>
__global__ __launch_bounds__(256) void k_small_linear_bwd(const float* __restrict__ g, const float* __restrict__ x,
                                                          const float* __restrict__ w, float* __restrict__ g_x,
                                                          float* __restrict__ dW, float* __restrict__ db, int64_t M, int K, int C,
                                                          int64_t rows_per_chunk, float gate_scale, const fn_head_act below) {
    // blockIdx.y = row chunk: dW / db then point at per-chunk partials [chunk][C*K] / [chunk][C] (k_sum_chunks finishes)
    __shared__ float4 sm[64][4];
    __shared__ float s_slope[4];
    const int c4 = threadIdx.x & 3, rl = threadIdx.x >> 2;           // 4 float4 columns x 64 row lanes
    const int col = blockIdx.x * 16 + c4 * 4;
    const bool live = col < K;
    const int64_t m_begin = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t m_end = m_begin + rows_per_chunk < M ? m_begin + rows_per_chunk : M;
    dW += (size_t)blockIdx.y * C * K;
    db += (size_t)blockIdx.y * C;
    float4 wv[CM], acc[CM];
    HactRun hr{};
    if (HACT) hr = hact_run(below, below.kind);
    float dslope = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        wv[c] = (live && c < C) ? ld4(w + (size_t)c * K + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (live) {
        // U rows per trip (four; two for the widest class: registers), every load issued before the first use (one row per trip made the 512-row head a chain of
        // eight dependent round trips: 7.4 us for 1 MB)
        constexpr int U = CM > 4 ? 2 : 4;
        for (int64_t m0 = m_begin + rl; m0 < m_end; m0 += U * 64) {
            float4 xv[U];
            float gv[U][CM];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t m = m0 + 64 * u < m_end ? m0 + 64 * u : m0;
                xv[u] = ld4(x + m * K + col);
#pragma unroll
                for (int c = 0; c < CM; ++c) gv[u][c] = c < C ? g[m * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t m = m0 + 64 * u;
                if (m >= m_end) continue;
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C) {
                        o.x += gv[u][c] * wv[c].x; o.y += gv[u][c] * wv[c].y; o.z += gv[u][c] * wv[c].z; o.w += gv[u][c] * wv[c].w;
                        acc[c].x += gv[u][c] * xv[u].x; acc[c].y += gv[u][c] * xv[u].y; acc[c].z += gv[u][c] * xv[u].z; acc[c].w += gv[u][c] * xv[u].w;
                    }
                }
                if (HACT) o = hact_bwd4_rt(below, hr, o, ld4(below.pre + m * K + col), (uint64_t)(m * K + col), dslope);
                else if (gate_scale > 0.f) {                        // x = relu(dropout(.)) of the layer below: its backward, fused
                    o.x = xv[u].x > 0.f ? o.x * gate_scale : 0.f;  o.y = xv[u].y > 0.f ? o.y * gate_scale : 0.f;
                    o.z = xv[u].z > 0.f ? o.z * gate_scale : 0.f;  o.w = xv[u].w > 0.f ? o.w * gate_scale : 0.f;
                }
                st4(g_x + m * K + col, o);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < C) {                                                // uniform
            sm[rl][c4] = acc[c];
            __syncthreads();
            if (rl == 0 && live) {
                float4 t = sm[0][c4];
                for (int q = 1; q < 64; ++q) { const float4 u = sm[q][c4]; t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
                st4(dW + (size_t)c * K + col, t);
            }
            __syncthreads();
        }
    }
    if (blockIdx.x == 0) {                                          // bias gradient: one wave per class, fixed order
        const int lane = threadIdx.x & 63;
        for (int c = threadIdx.x >> 6; c < C; c += 4) {
            float t = 0.f;
            for (int64_t m = m_begin + lane; m < m_end; m += 64) t += g[m * C + c];
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (lane == 0) db[c] = t;
        }
    }
    if (HACT && below.kind == FN_ACT_PRELU) hact_block_partial<4>(dslope, below.part, (int)(blockIdx.y * gridDim.x + blockIdx.x), s_slope);
}

// The last Linear of a head, the loss on its outputs and that Linear's INPUT gradient in one launch (round 4; VERDICT r3 item 4: three
// dependent launches of 4-6 us each were one row-local computation apart from two sums).  Once the loss's denominator is known -- it
// depends on the row weights / label mask only, never on the predictions, so every block recomputes it from L2 (a few KB) -- a row's
// prediction, its loss gradient g = dL/dy and its input gradient g_x = g w (gated by x > 0) need nothing from other rows: one wave per
// row, the row in registers throughout.  What does cross rows is left as data for the next launch (the head's first fn_dense_bwd
// call carries the blocks, dense_head.inc small_dw_*): dW = g^T x, db = colsum(g), and the loss value as per-block partial sums
// (already divided by the denominator).  No ticket, no atomic: fixed-order sums only.  Numbers: y, g, g_x are bit-identical to
// fn_small_linear_f32 -> fn_masked_mse/bce_f32 -> fn_small_linear_bwd_f32 (same operation order).
// HACT: g_x goes through the activation kind `below` (head_act.inc) instead of the ReLU gate.
template <int CM, bool HACT>
__global__ __launch_bounds__(256) void k_small_linear_loss(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                           const float* __restrict__ target, const float* __restrict__ row_w, const int kind,
                                                           float* __restrict__ y, float* __restrict__ g, float* __restrict__ g_x,
                                                           const float gate_scale, float* __restrict__ loss_part, const int64_t M, const int K,
                                                           const int C, const int64_t M_out, const fn_head_act below) {
    __shared__ float s4[4], s_slope[4];
    HactRun hr{};
    if (HACT) hr = hact_run(below, below.kind);
    float dslope = 0.f;
    __shared__ float sden;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float cnt = 0.f;
    if (kind == FN_LOSS_MSE) {
        for (int64_t i = threadIdx.x; i < M_out; i += 256) cnt += row_w[i];
    } else {
        for (int64_t i = threadIdx.x; i < M_out * C; i += 256) cnt += (target[i] > -0.5f && row_w[i / C] > 0.f) ? 1.f : 0.f;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) s4[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) sden = ((s4[0] + s4[1]) + (s4[2] + s4[3])) * (kind == FN_LOSS_MSE ? (float)C : 1.f);
    __syncthreads();
    const float den = sden;
    const int64_t row = (int64_t)blockIdx.x * 4 + wv;
    const int k4 = K / 4;                                            // K % 4 == 0, K <= 1024: four 16-byte pieces per lane at most
    float lsum = 0.f;
    if (row < M) {
        float4 xv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;
            xv[q] = j < k4 ? ld4(x + row * K + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float wm = row_w[row];
        float gc[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            gc[c] = 0.f;
            if (c < C) {                                             // uniform
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int j = lane + 64 * q;
                    if (j < k4) acc += dot4(xv[q], ld4(w + (size_t)c * K + 4 * j));
                }
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
                const float yv = acc + (b ? b[c] : 0.f), t = target[row * C + c];
                if (kind == FN_LOSS_MSE) {
                    const float d = yv - t, scale = 2.f / den;
                    gc[c] = scale * wm * d;
                    lsum = fmaf(wm * d, d, lsum);
                } else if (t > -0.5f && wm > 0.f) {
                    const float tt = fmaxf(t, 0.f);
                    lsum += fmaxf(yv, 0.f) - yv * tt + log1pf(expf(-fabsf(yv)));
                    gc[c] = (1.f / (1.f + expf(-yv)) - tt) * (1.f / den);
                }
                if (lane == 0) { y[row * C + c] = yv;  g[row * C + c] = gc[c]; }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + 64 * q;
            if (j < k4) {
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    if (c < C) {
                        const float4 wc = ld4(w + (size_t)c * K + 4 * j);
                        o.x += gc[c] * wc.x; o.y += gc[c] * wc.y; o.z += gc[c] * wc.z; o.w += gc[c] * wc.w;
                    }
                }
                if (HACT) o = hact_bwd4_rt(below, hr, o, ld4(below.pre + row * K + 4 * j), (uint64_t)(row * K + 4 * j), dslope);
                else if (gate_scale > 0.f) {                         // x = relu(dropout(.)) of the layer below: its backward, fused
                    o.x = xv[q].x > 0.f ? o.x * gate_scale : 0.f;  o.y = xv[q].y > 0.f ? o.y * gate_scale : 0.f;
                    o.z = xv[q].z > 0.f ? o.z * gate_scale : 0.f;  o.w = xv[q].w > 0.f ? o.w * gate_scale : 0.f;
                }
                st4(g_x + row * K + 4 * j, o);
            }
        }
    } else if (row < M_out && lane < C) {
        y[row * C + lane] = 0.f;                                     // padding rows of a static-shape batch: defined, 0
    }
    if (lane == 0) s4[wv] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) loss_part[blockIdx.x] = ((s4[0] + s4[1]) + (s4[2] + s4[3])) / den;
    if (HACT && below.kind == FN_ACT_PRELU) hact_block_partial<4>(dslope, below.part, (int)blockIdx.x, s_slope);
}

#include "dense_head.inc"

constexpr int64_t kTallRows = 2048, kTallChunk = 256;      // inputs taller than kTallRows are reduced in chunks of kTallChunk rows
inline int64_t tall_chunks(int64_t rows) { return rows > kTallRows ? (rows + kTallChunk - 1) / kTallChunk : 1; }
// the CM template argument of k_small_linear_bwd / k_small_linear_loss: f(CM) for the smallest of 1, 4, FN_SMALL_LINEAR_MAX that holds C classes
template <class F> inline void with_small_cm(int64_t C, F&& f) { with_const<1, 4, FN_SMALL_LINEAR_MAX>(C <= 1 ? 1 : C <= 4 ? 4 : FN_SMALL_LINEAR_MAX, f); }
// the instance of a dense kernel for a head activation kind: what f(HA) hands back for HA = ha (-1, also for anything else: the ReLU
// path of fn_act_epilogue / gate_scale)
template <class F> inline auto with_head_kind(int ha, F&& f) {
    auto k = f(std::integral_constant<int, -1>{});
    with_const<FN_ACT_RELU, FN_ACT_SILU, FN_ACT_GELU, FN_ACT_CELU, FN_ACT_SELU, FN_ACT_RELU6, FN_ACT_LEAKYRELU, FN_ACT_PRELU>(ha, [&](auto HA) { k = f(HA); });
    return k;
}
}  // namespace

extern "C" {

int64_t fn_gate_colsum_ws(int64_t rows, int64_t cols) {
    const int64_t ch = tall_chunks(rows);
    return ch > 1 ? ch * cols : 0;
}

int fn_gate_colsum_f32(const float* g_y, const float* y, float* g_x, float* colsum, int64_t rows, int64_t cols, float scale,
                       float* ws, fn_stream_t stream) {
    if (rows < 0 || cols < 0 || (cols & 3) || cols > INT32_MAX) return fail(FN_EINVAL, "fn_gate_colsum_f32: cols must be a multiple of 4");
    if (cols == 0) return 0;
    if (!colsum || (rows > 0 && (!g_y || !y || !g_x)) || (((uintptr_t)g_y | (uintptr_t)y | (uintptr_t)g_x | (uintptr_t)colsum | (uintptr_t)ws) & 15))
        return fail(FN_EINVAL, "fn_gate_colsum_f32: null or misaligned buffer");
    const int64_t ch = tall_chunks(rows);
    if (ch > 1 && !ws) return fail(FN_EINVAL, "fn_gate_colsum_f32: rows > 2048 need the fn_gate_colsum_ws() workspace");
    hipLaunchKernelGGL(k_gate_colsum, dim3((unsigned)((cols + 31) / 32), (unsigned)ch), dim3(256), 0, S(stream), g_y, y, g_x,
                       ch > 1 ? ws : colsum, rows, (int)cols, scale, ch > 1 ? kTallChunk : (rows > 0 ? rows : 1));
    if (ch > 1) hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)((cols + 15) / 16)), dim3(256), 0, S(stream), ws, (int)ch, cols, colsum);
    return launch_status("fn_gate_colsum_f32");
}

int fn_small_linear_f32(const float* x, const float* w, const float* b, float* y, int64_t M, int64_t K, int64_t C, int64_t M_out,
                        fn_stream_t stream) {
    if (M < 0 || K < 4 || (K & 3) || K > INT32_MAX || C < 1 || C > FN_SMALL_LINEAR_MAX)
        return fail(FN_EINVAL, "fn_small_linear_f32: K must be a multiple of 4 and 1 <= C <= FN_SMALL_LINEAR_MAX");
    if (M_out < M) M_out = M;
    if (M_out == 0) return 0;
    if (!x || !w || !y || (((uintptr_t)x | (uintptr_t)w) & 15)) return fail(FN_EINVAL, "fn_small_linear_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_small_linear, dim3((unsigned)((M_out + 3) / 4)), dim3(256), 0, S(stream), x, w, b, y, M, (int)K, (int)C, M_out);
    return launch_status("fn_small_linear_f32");
}

int64_t fn_small_linear_bwd_ws(int64_t M, int64_t K, int64_t C) {
    const int64_t ch = tall_chunks(M);
    return ch > 1 ? ch * C * (K + 1) : 0;
}

// the activation handed to a backward as `below`: a known kind and order, its saved argument, the PReLU slope and partials
static bool head_act_ok(const fn_head_act* h, bool need_part) {
    return h->kind >= FN_ACT_RELU && h->kind <= FN_ACT_PRELU && (h->order == FN_ACT_DROP_THEN_ACT || h->order == FN_ACT_ACT_THEN_DROP) &&
           h->p >= 0.f && h->p <= 1.f && h->pre && !((uintptr_t)h->pre & 15) &&
           (h->kind != FN_ACT_PRELU || (h->prelu_w && (!need_part || h->part)));
}

static int small_linear_bwd(const float* g, const float* x, const float* w, float* g_x, float* dW, float* db, int64_t M, int64_t K,
                            int64_t C, float gate_scale, const fn_head_act* below, float* ws, fn_stream_t stream) {
    if (below && !head_act_ok(below, true)) return fail(FN_EINVAL, "fn_small_linear_bwd_act_f32: bad activation");
    if (M < 0 || K < 4 || (K & 3) || K > INT32_MAX || C < 1 || C > FN_SMALL_LINEAR_MAX)
        return fail(FN_EINVAL, "fn_small_linear_bwd_f32: K must be a multiple of 4 and 1 <= C <= FN_SMALL_LINEAR_MAX");
    if (!w || !dW || !db || (M > 0 && (!g || !x || !g_x)) || (((uintptr_t)x | (uintptr_t)w | (uintptr_t)g_x | (uintptr_t)dW | (uintptr_t)ws) & 15))
        return fail(FN_EINVAL, "fn_small_linear_bwd_f32: null or misaligned buffer");
    const int64_t ch = tall_chunks(M);
    if (ch > 1 && !ws) return fail(FN_EINVAL, "fn_small_linear_bwd_f32: M > 2048 needs the fn_small_linear_bwd_ws() workspace");
    float* dW_o = ch > 1 ? ws : dW;
    float* db_o = ch > 1 ? ws + ch * C * K : db;
    const int64_t rpc = ch > 1 ? kTallChunk : (M > 0 ? M : 1);
    const dim3 grid((unsigned)((K + 15) / 16), (unsigned)ch);
    const fn_head_act h = below ? *below : fn_head_act{};
    with_small_cm(C, [&](auto CM) { with_const<0, 1>(below && M > 0, [&](auto HACT) {      // (without rows there is nothing to put through `below`)
        hipLaunchKernelGGL((k_small_linear_bwd<FN_CV(CM), FN_CV(HACT) != 0>), grid, dim3(256), 0, S(stream), g, x, w, g_x, dW_o, db_o, M, (int)K, (int)C, rpc, gate_scale, h);
    }); });
    if (ch > 1) {
        hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)((C * K + 15) / 16)), dim3(256), 0, S(stream), ws, (int)ch, C * K, dW);
        hipLaunchKernelGGL(k_sum_chunks, dim3((unsigned)((C + 15) / 16)), dim3(256), 0, S(stream), ws + ch * C * K, (int)ch, C, db);
    }
    return launch_status("fn_small_linear_bwd_f32");
}

int fn_small_linear_bwd_f32(const float* g, const float* x, const float* w, float* g_x, float* dW, float* db, int64_t M, int64_t K,
                            int64_t C, float gate_scale, float* ws, fn_stream_t stream) {
    return small_linear_bwd(g, x, w, g_x, dW, db, M, K, C, gate_scale, nullptr, ws, stream);
}

int fn_small_linear_bwd_act_f32(const float* g, const float* x, const float* w, float* g_x, float* dW, float* db, int64_t M, int64_t K,
                                int64_t C, const fn_head_act* below, float* ws, fn_stream_t stream) {
    return small_linear_bwd(g, x, w, g_x, dW, db, M, K, C, 0.f, below, ws, stream);
}

int64_t fn_small_linear_loss_ws(int64_t M_out) { return M_out > 0 ? (M_out + 3) / 4 : 0; }

static int small_linear_loss(const float* x, const float* w, const float* b, const float* target, const float* row_w, int kind,
                             float* y, float* g, float* g_x, float gate_scale, const fn_head_act* below, float* loss_part, int64_t M,
                             int64_t K, int64_t C, int64_t M_out, fn_stream_t stream) {
    if (below && !head_act_ok(below, true)) return fail(FN_EINVAL, "fn_small_linear_loss_act_f32: bad activation");
    if (M < 0 || K < 4 || (K & 3) || K > FN_SMALL_LINEAR_LOSS_MAX_K || C < 1 || C > FN_SMALL_LINEAR_MAX || (kind != FN_LOSS_MSE && kind != FN_LOSS_BCE))
        return fail(FN_EINVAL, "fn_small_linear_loss_f32: K a multiple of 4 and <= FN_SMALL_LINEAR_LOSS_MAX_K, 1 <= C <= FN_SMALL_LINEAR_MAX, kind MSE or BCE");
    if (M_out < M) M_out = M;
    if (M_out == 0) return 0;
    if (!w || !target || !row_w || !y || !loss_part || gate_scale < 0.f || (M > 0 && (!x || !g || !g_x)) ||
        (((uintptr_t)x | (uintptr_t)w | (uintptr_t)g_x) & 15))
        return fail(FN_EINVAL, "fn_small_linear_loss_f32: null or misaligned buffer");
    const dim3 grid((unsigned)fn_small_linear_loss_ws(M_out));
    const fn_head_act h = below ? *below : fn_head_act{};
    with_small_cm(C, [&](auto CM) { with_const<0, 1>(below != nullptr, [&](auto HACT) {
        hipLaunchKernelGGL((k_small_linear_loss<FN_CV(CM), FN_CV(HACT) != 0>), grid, dim3(256), 0, S(stream), x, w, b, target, row_w, kind, y, g, g_x, gate_scale, loss_part, M, (int)K, (int)C, M_out, h);
    }); });
    return launch_status("fn_small_linear_loss_f32");
}

int fn_small_linear_loss_f32(const float* x, const float* w, const float* b, const float* target, const float* row_w, int kind,
                             float* y, float* g, float* g_x, float gate_scale, float* loss_part, int64_t M, int64_t K, int64_t C,
                             int64_t M_out, fn_stream_t stream) {
    return small_linear_loss(x, w, b, target, row_w, kind, y, g, g_x, gate_scale, nullptr, loss_part, M, K, C, M_out, stream);
}

int fn_small_linear_loss_act_f32(const float* x, const float* w, const float* b, const float* target, const float* row_w, int kind,
                                 float* y, float* g, float* g_x, const fn_head_act* below, float* loss_part, int64_t M, int64_t K,
                                 int64_t C, int64_t M_out, fn_stream_t stream) {
    return small_linear_loss(x, w, b, target, row_w, kind, y, g, g_x, 0.f, below, loss_part, M, K, C, M_out, stream);
}

// (static, not an anonymous namespace: inside this extern "C" block clang gives a namespace-scope function C linkage and exports it)
static bool dense_shape_ok(int64_t M, int64_t K, int64_t N) {
    return M >= 0 && M <= FN_DENSE_MAX_ROWS && K >= 4 && N >= 4 && !(K & 3) && !(N & 3) && K <= 65536 && N <= 65536;
}
static int dense_tiles(int64_t n, int t) { return (int)((n + t - 1) / t); }

// the instances of a head activation kind (HA = -1: the ReLU path of fn_act_epilogue / gate_scale)
typedef void (*DenseFwdK)(const DenseArgs, const int);
typedef void (*DenseTilesK)(const DenseArgs);
typedef void (*DenseBwdK)(const DensePair, const SmallDw);
static DenseFwdK dense_fwd_k(int ha) { return with_head_kind(ha, [](auto HA) -> DenseFwdK { return k_dense_fwd<FN_CV(HA)>; }); }
static DenseTilesK dense_tiles_k(int ha) { return with_head_kind(ha, [](auto HA) -> DenseTilesK { return k_dense_fwd_tiles<FN_CV(HA)>; }); }
static DenseBwdK dense_bwd_k(int ha) { return with_head_kind(ha, [](auto HA) -> DenseBwdK { return k_dense_bwd<FN_CV(HA)>; }); }

static int dense_fwd(const float* X, const float* W, const float* bias, float* Y, int64_t M, int64_t K, int64_t N,
                     const fn_act_epilogue* act, const fn_head_act* hact, fn_stream_t stream) {
    if (!dense_shape_ok(M, K, N)) return fail(FN_EINVAL, "fn_dense_fwd_f32: K and N must be multiples of 4, M <= FN_DENSE_MAX_ROWS");
    if (M == 0) return 0;
    if (!X || !W || !Y || (((uintptr_t)X | (uintptr_t)W | (uintptr_t)Y | (uintptr_t)bias) & 15))
        return fail(FN_EINVAL, "fn_dense_fwd_f32: null or misaligned buffer");
    if (act && (act->p < 0.f || act->p > 1.f)) return fail(FN_EINVAL, "fn_dense_fwd_f32: dropout probability outside [0, 1]");
    if (hact && !head_act_ok(hact, false)) return fail(FN_EINVAL, "fn_dense_fwd_act_f32: bad activation (kind, order, p, pre, prelu_w)");
    DenseArgs T{};
    T.A = X;  T.Bsrc = W;  T.bias = bias;  T.OUT = Y;
    T.I = (int)M;  T.J = (int)N;  T.R = (int)K;  T.lda = (int)K;  T.ldb = (int)K;
    if (act) { T.act = *act;  T.act.y = Y; }
    const int ha = hact ? hact->kind : -1;
    if (hact) T.hact = *hact;
    // tall inputs: workgroup-shared 64 x 128 operand tiles (dense_head.inc, k_dense_fwd_tiles).  32-bit element offsets as elsewhere
    if (tune(FN_TUNE_DENSE_TILES) != 0 && K % kDtK == 0 && dense_tiles(M, kDtM) * dense_tiles(N, kDtN) >= kDtMinTiles) {
        T.tiles_i = dense_tiles(M, kDtM);  T.tiles_j = dense_tiles(N, kDtN);
        const DenseTilesK kern = dense_tiles_k(ha);
        if (int rc = allow_lds(kern, kDtLdsBytes)) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)(8 * ((T.tiles_i * T.tiles_j + 7) / 8))), dim3(kDtThreads), kDtLdsBytes, S(stream), T);
        return launch_status("fn_dense_fwd_f32 (workgroup-shared tiles)");
    }
    T.tiles_i = dense_tiles(M, 32);  T.tiles_j = dense_tiles(N, kDnCols);
    const int narrow = T.tiles_i * T.tiles_j < 192;      // too few 32 x 64 tiles to occupy the chip: 32 x 32
    if (narrow) T.tiles_j = dense_tiles(N, 32);
    hipLaunchKernelGGL(dense_fwd_k(ha), dim3((unsigned)(T.tiles_i * T.tiles_j)), dim3(kDnThreads), kDnLdsBytes, S(stream), T, narrow);
    return launch_status("fn_dense_fwd_f32");
}

int fn_dense_fwd_f32(const float* X, const float* W, const float* bias, float* Y, int64_t M, int64_t K, int64_t N,
                     const fn_act_epilogue* act, fn_stream_t stream) {
    return dense_fwd(X, W, bias, Y, M, K, N, act, nullptr, stream);
}

int fn_dense_fwd_act_f32(const float* X, const float* W, const float* bias, float* Y, int64_t M, int64_t K, int64_t N,
                         const fn_head_act* act, fn_stream_t stream) {
    if (!act) return fail(FN_EINVAL, "fn_dense_fwd_act_f32: act is required");
    return dense_fwd(X, W, bias, Y, M, K, N, nullptr, act, stream);
}

int fn_dense_bwd_f32(const float* g_y, const float* X, const float* W, float* g_x, float gate_scale, float* dW, float* db,
                     int64_t M, int64_t K, int64_t N, int64_t M_out, fn_stream_t stream) {
    return fn_dense_bwd_tail_f32(g_y, X, W, g_x, gate_scale, dW, db, M, K, N, M_out, nullptr, stream);
}

// the DX tiles of a dense backward with M_out rows and K input features (the tiling below)
static void dense_dx_tiles(int64_t M_out, int64_t K, int* tiles_i, int* tiles_j, int* narrow) {
    *tiles_i = dense_tiles(M_out, 32);  *tiles_j = dense_tiles(K, kDnCols);  *narrow = 0;
    if (*tiles_i * *tiles_j < 192) { *narrow = 1;  *tiles_j = dense_tiles(K, 32); }
}

static int dense_bwd(const float* g_y, const float* X, const float* W, float* g_x, float gate_scale, const fn_head_act* below, float* dW,
                     float* db, int64_t M, int64_t K, int64_t N, int64_t M_out, const fn_small_dw* tail, fn_stream_t stream) {
    if (below && !head_act_ok(below, true)) return fail(FN_EINVAL, "fn_dense_bwd_act_f32: bad activation (kind, order, p, pre, prelu_w, part)");
    if (!dense_shape_ok(M, K, N)) return fail(FN_EINVAL, "fn_dense_bwd_f32: K and N must be multiples of 4, M <= FN_DENSE_MAX_ROWS");
    SmallDw sd{};
    sd.first_block = -1;
    if (tail) {
        if (tail->M < 0 || tail->M > FN_DENSE_MAX_ROWS || tail->K < 4 || (tail->K & 3) || tail->K > 65536 || tail->C < 1 ||
            tail->C > FN_SMALL_LINEAR_MAX || tail->n_part < 0 || !tail->dW || !tail->db || (tail->M > 0 && (!tail->g || !tail->x)) ||
            (tail->loss && tail->n_part > 0 && !tail->loss_part) || (((uintptr_t)tail->x | (uintptr_t)tail->dW) & 15))
            return fail(FN_EINVAL, "fn_dense_bwd_tail_f32: bad tail (M <= FN_DENSE_MAX_ROWS, K % 4 == 0, 1 <= C <= FN_SMALL_LINEAR_MAX)");
        sd.g = tail->g;  sd.x = tail->x;  sd.dW = tail->dW;  sd.db = tail->db;  sd.loss_part = tail->loss_part;  sd.loss = tail->loss;
        sd.n_part = (int)tail->n_part;  sd.M = (int)tail->M;  sd.K = (int)tail->K;  sd.C = (int)tail->C;
    }
    if (!W || !dW || (M > 0 && (!g_y || !X)) || gate_scale < 0.f ||
        (((uintptr_t)g_y | (uintptr_t)X | (uintptr_t)W | (uintptr_t)g_x | (uintptr_t)dW) & 15))
        return fail(FN_EINVAL, "fn_dense_bwd_f32: null or misaligned buffer");
    DensePair P{};
    DenseArgs& a = P.a;                                  // dW [N,K] = gy^T X, db = column sums of gy
    a.A = g_y;  a.Bsrc = X;  a.OUT = dW;  a.db = db;
    a.I = (int)N;  a.J = (int)K;  a.R = (int)M;  a.lda = (int)N;  a.ldb = (int)K;
    a.tiles_i = dense_tiles(N, 64);  a.tiles_j = dense_tiles(K, kDnCols);
    if (a.tiles_i * a.tiles_j < 192) {                   // too few 64 x 64 tiles to occupy the chip: 64 x 32 tiles (dense_dw_narrow)
        P.a_narrow = 1;
        a.tiles_j = dense_tiles(K, 32);
    }
    int blocks = a.tiles_i * a.tiles_j;
    P.b.first_block = blocks;
    int ha = -1;                                         // the instance: the layer below's activation kind once there is an input gradient
    if (M_out < M) M_out = M;
    if (M_out > FN_DENSE_MAX_ROWS) return fail(FN_EINVAL, "fn_dense_bwd_f32: M_out > FN_DENSE_MAX_ROWS");
    if (g_x && M_out > 0 && M == 0) {                    // no input rows: the padding rows of g_x are all there is, and they are zero
        hipLaunchKernelGGL(k_zero2_i32, dim3(flat_grid(M_out * K, kGridCap)), dim3(kBlock), 0, S(stream),
                           reinterpret_cast<int32_t*>(g_x), M_out * K, static_cast<int32_t*>(nullptr), (int64_t)0);
        if (int rc = launch_status("fn_dense_bwd_f32 (empty input)")) return rc;
    } else if (g_x && M_out > 0) {
        DenseArgs& b = P.b;                              // gX [M,K] = gy W, gated by X > 0
        b.A = g_y;  b.Bsrc = W;  b.OUT = g_x;  b.Z = gate_scale > 0.f ? X : nullptr;  b.gate_scale = gate_scale;
        b.I = (int)M;  b.I_out = (int)M_out;  b.J = (int)K;  b.R = (int)N;  b.lda = (int)N;  b.ldb = (int)K;
        if (below) ha = below->kind, b.hact = *below;
        dense_dx_tiles(M_out, K, &b.tiles_i, &b.tiles_j, &P.b_narrow);
        blocks += b.tiles_i * b.tiles_j;
    }
    if (tail) {
        sd.first_block = blocks;
        blocks += (sd.K + 15) / 16 + 1;
    }
    hipLaunchKernelGGL(dense_bwd_k(ha), dim3((unsigned)blocks), dim3(kDnThreads), kDnLdsBytes, S(stream), P, sd);
    return launch_status("fn_dense_bwd_f32");
}

int fn_dense_bwd_tail_f32(const float* g_y, const float* X, const float* W, float* g_x, float gate_scale, float* dW, float* db,
                          int64_t M, int64_t K, int64_t N, int64_t M_out, const fn_small_dw* tail, fn_stream_t stream) {
    return dense_bwd(g_y, X, W, g_x, gate_scale, nullptr, dW, db, M, K, N, M_out, tail, stream);
}

int fn_dense_bwd_act_f32(const float* g_y, const float* X, const float* W, float* g_x, const fn_head_act* below, float* dW, float* db,
                         int64_t M, int64_t K, int64_t N, int64_t M_out, const fn_small_dw* tail, fn_stream_t stream) {
    return dense_bwd(g_y, X, W, g_x, 0.f, below, dW, db, M, K, N, M_out, tail, stream);
}

int64_t fn_head_act_parts(int where, int64_t rows, int64_t K) {
    if (rows <= 0 || K <= 0) return 0;
    if (where == FN_ACT_AT_SMALL_LOSS) return fn_small_linear_loss_ws(rows);
    if (where == FN_ACT_AT_SMALL_BWD) return ((K + 15) / 16) * tall_chunks(rows);
    int ti, tj, narrow;
    dense_dx_tiles(rows, K, &ti, &tj, &narrow);
    return (int64_t)ti * tj;
}

int fn_head_act_param_grad_f32(const float* part, int64_t n, float* grad, fn_stream_t stream) {
    if (n < 0 || !grad || (n > 0 && !part)) return fail(FN_EINVAL, "fn_head_act_param_grad_f32: bad argument");
    hipLaunchKernelGGL(k_head_act_param_grad, dim3(1), dim3(256), 0, S(stream), part, n, grad);
    return launch_status("fn_head_act_param_grad_f32");
}
}  // extern "C"
