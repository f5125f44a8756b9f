// param_grads.hip -- the parameter-gradient family: everything that turns a backward pass's rows and per-block partials into the
// gradients of the encoder's PARAMETERS.  The weight-gradient partial products dW = dY^T X of the projections (wgrad_body: k_linear128_wgrad,
// _multi, _mixed; the direct K = 128 form of wgrad128.inc; k_wgrad_all), the reductions of partials (k_wgrad_reduce; the deferred task
// table k_reduce_tasks with the attention vectors' / edge embeddings' finalize and the column sums of the edge term), and the host object
// that batches them for the engine, fni::ParamGradQueue (fn_internal.h).  The stand-alone operators on the same bodies live here too:
// fn_linear128_wgrad_f32 / _ws and fn_gat_bwd_finalize_f32.
// A translation unit of its own: nothing here runs a device body that a kernel of another unit runs, except adam_ride (shared_bodies.inc:
// the Adam rider of k_reduce_tasks, which the fragment tail's backward kernel in encoder.hip can carry instead;
// profiles/param_grads_unit_equivalence.txt), and the host code needs pointers and counts only: the queue's methods take plain argument
// structs, never a type of the engine.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;
using fni::tune;
using fni::ReduceTask;
using fni::ReduceTasks;
using fni::WgradTask;
using fni::WgradTasks;
using fni::kMaxReduceTasks;
using fni::kMaxWgradTasks;
using fni::RT_FINALIZE;
using fni::RT_COLSUM;
using fni::RT_WGRAD;

#include "zero2.inc"
#include "shared_bodies.inc"
#include "linear128.inc"      // kBtLd: the partial products stage dY with the leading dimension of the projections' LDS operand

// Weight gradient: block = `rows_per_block` rows in chunks of 32 staged through double-buffered LDS.  Wave w owns
// output rows o in [32(w&3), +32) and the (w>>2)-th group of CTW 16-column tiles of X, so NH = 2 column groups
// put two waves on every SIMD.  part [grid][128*K + 128]: dW partial followed by the db partial.
constexpr int kWgChunk = 32;
template <int CTW, int NH>
__device__ __forceinline__ void wgrad_body(float* smem, const float* __restrict__ dY, const float* __restrict__ X, int K,
                                           int64_t M, int rows_per_block, float* __restrict__ part, int bid) {
    constexpr int NT = 256 * NH;
    constexpr int XW = 16 * CTW * NH;            // padded X width held in LDS
    constexpr int XLD = XW + 16;                 // XW is a multiple of 32 for every instantiation but <1,1>
    float* sY = smem;                                   // [2][32][144]
    float* sX = smem + 2 * kWgChunk * kBtLd;            // [2][32][XLD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, kq = lane >> 4;
    const int wo = w & 3, wc = w >> 2;
    const int64_t m_begin = (int64_t)bid * rows_per_block;
    const int64_t m_end = m_begin + rows_per_block < M ? m_begin + rows_per_block : M;
    const int n_chunks = (int)((m_end - m_begin + kWgChunk - 1) / kWgChunk);

    constexpr int YPT = 1024 / NT;                            // dY float4 per thread per chunk
    constexpr int XPT = (kWgChunk * XW + NT - 1) / NT;        // X scalars per thread per chunk
    float4 ry[YPT];
    float rx[XPT];
    auto fetch = [&](int c) {
        const int64_t base = m_begin + (int64_t)c * kWgChunk;
#pragma unroll
        for (int q = 0; q < YPT; ++q) {
            const int idx = tid + q * NT, r = idx >> 5, c4 = idx & 31;
            ry[q] = (base + r < m_end) ? ld4(dY + (base + r) * 128 + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < XPT; ++q) {
            const int idx = tid + q * NT, r = idx / XW, cc = idx % XW;
            rx[q] = (r < kWgChunk && base + r < m_end && cc < K) ? X[(base + r) * K + cc] : 0.f;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < YPT; ++q) {
            const int idx = tid + q * NT, r = idx >> 5, c4 = idx & 31;
            st4(sY + (buf * kWgChunk + r) * kBtLd + c4 * 4, ry[q]);
        }
#pragma unroll
        for (int q = 0; q < XPT; ++q) {
            const int idx = tid + q * NT, r = idx / XW, cc = idx % XW;
            if (r < kWgChunk) sX[(buf * kWgChunk + r) * XLD + cc] = rx[q];
        }
    };

    f32x4 acc[2][CTW];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int c = 0; c < CTW; ++c) acc[u][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum[2] = {0.f, 0.f};

    if (n_chunks > 0) { fetch(0); stash(0); }
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < n_chunks) fetch(c + 1);
#pragma unroll
        for (int s = 0; s < kWgChunk / 4; ++s) {
            const float* yrow = sY + (buf * kWgChunk + 4 * s + kq) * kBtLd + 32 * wo + i;
            const float* xrow = sX + (buf * kWgChunk + 4 * s + kq) * XLD + 16 * CTW * wc + i;
            const float a0 = yrow[0], a1 = yrow[16];
            bsum[0] += a0;
            bsum[1] += a1;
            float bv[CTW];
#pragma unroll
            for (int cc = 0; cc < CTW; ++cc) bv[cc] = xrow[16 * cc];
#pragma unroll
            for (int cc = 0; cc < CTW; ++cc) {
                acc[0][cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv[cc], acc[0][cc], 0, 0, 0);
                acc[1][cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv[cc], acc[1][cc], 0, 0, 0);
            }
        }
        if (c + 1 < n_chunks) stash(buf ^ 1);
        __syncthreads();
    }
    // partials are written in the accumulators' native layout: one coalesced 16-byte store per lane and tile;
    // k_wgrad_reduce maps them back to dW[o][col] while summing over blocks
    constexpr int PW = 128 * XW + 128;
    float* pw = part + (size_t)bid * PW;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int cc = 0; cc < CTW; ++cc)
            st4(pw + ((size_t)((w * 2 + u) * CTW + cc) * 64 + lane) * 4,
                make_float4(acc[u][cc][0], acc[u][cc][1], acc[u][cc][2], acc[u][cc][3]));
    if (wc == 0) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float v = bsum[u];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (kq == 0) pw[(size_t)128 * XW + 32 * wo + 16 * u + i] = v;
        }
    }
}

template <int CTW, int NH>
__global__ __launch_bounds__(256 * NH) void k_linear128_wgrad(const float* __restrict__ dY, const float* __restrict__ X,
                                                              int K, int64_t M, int rows_per_block,
                                                              float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    wgrad_body<CTW, NH>(smem, dY, X, K, M, rows_per_block, part, (int)blockIdx.x);
}

// all weight-gradient partial products of a backward pass that share K (every projection beyond layer 0): one launch
// (WgradTask / WgradTasks: fn_internal.h)
#include "wgrad128.inc"
template <int CTW, int NH>
__global__ __launch_bounds__(256 * NH) void k_linear128_wgrad_multi(WgradTasks T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const WgradTask& t = T.t[ti];
    wgrad_body<CTW, NH>(smem, t.dY, t.X, T.K, t.M, t.rpb, t.part, (int)blockIdx.x - t.first);
}

// the weight-gradient partials of layer 0 (raw-feature widths: 17 / 6 / 167 at the reference's sizes) in one launch: every
// product picks the instantiation its K needs (all with two column groups, i.e. 512 threads); the launch's LDS size is the
// largest product's
__global__ __launch_bounds__(512) void k_linear128_wgrad_mixed(WgradTasks T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const WgradTask& t = T.t[ti];
    const int bid = (int)blockIdx.x - t.first;
    const int64_t M = t.n_real && *t.n_real < t.M ? (int64_t)*t.n_real : t.M;
    if (t.K <= 32) wgrad_body<1, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
    else if (t.K <= 128) wgrad_body<4, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
    else wgrad_body<6, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
}

// every weight-gradient partial product of a backward pass in ONE launch: blocks [0, n128) run the direct K = 128 kernel
// (csrc/wgrad128.inc, two row slices), the others layer 0's products; the launch's LDS size is the larger of the two needs.
// Neither group waits for the other, and the short layer-0 workgroups fill the CUs the long K = 128 ones leave towards the end.
__global__ __launch_bounds__(512) void k_wgrad_all(const WgradTasks W, const WgradTasks W0, int n128) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if ((int)blockIdx.x < n128) {
        int ti = 0;
        while (ti + 1 < W.n && (int)blockIdx.x >= W.t[ti + 1].first) ++ti;
        wgrad128_block<2>(W.t[ti], (int)blockIdx.x - W.t[ti].first, smem);
        return;
    }
    const int b = (int)blockIdx.x - n128;
    int ti = 0;
    while (ti + 1 < W0.n && b >= W0.t[ti + 1].first) ++ti;
    const WgradTask& t = W0.t[ti];
    const int bid = b - t.first;
    const int64_t M = t.n_real && *t.n_real < t.M ? (int64_t)*t.n_real : t.M;
    if (t.K <= 32) wgrad_body<1, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
    else if (t.K <= 128) wgrad_body<4, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
    else wgrad_body<6, 2>(smem, t.dY, t.X, t.K, M, t.rpb, t.part, bid);
}

// sums the native-layout partials over blocks and scatters them to dW [128][K] / db [128]
template <int CTW, int NH>
__device__ __forceinline__ void wgrad_reduce_body(int vb, float* sm, const float* __restrict__ part, int n_rows, int K,
                                                  float* __restrict__ dW, float* __restrict__ db) {
    constexpr int XW = 16 * CTW * NH;
    constexpr int PW = 128 * XW + 128;
    float(*red)[33] = reinterpret_cast<float(*)[33]>(sm);
    const int c = threadIdx.x & 31, rg = threadIdx.x >> 5;
    const int col = vb * 32 + c;
    float acc = 0.f;
    if (col < PW)
        for (int r = rg; r < n_rows; r += 32) acc += part[(size_t)r * PW + col];
    red[rg][c] = acc;
    __syncthreads();
    if (threadIdx.x < 32 && col < PW) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < 32; ++g) v += red[g][threadIdx.x];
        if (col >= 128 * XW) {
            db[col - 128 * XW] = v;
        } else {
            const int r = col & 3, lane = (col >> 2) & 63, tile = col >> 8;        // tile = (w*2+u)*CTW + cc
            const int cc = tile % CTW, wu = tile / CTW, u = wu & 1, w = wu >> 1;
            const int o = 32 * (w & 3) + 16 * u + 4 * (lane >> 4) + r;
            const int xc = 16 * (CTW * (w >> 2) + cc) + (lane & 15);
            if (xc < K) dW[(size_t)o * K + xc] = v;
        }
    }
}

template <int CTW, int NH>
__global__ __launch_bounds__(1024) void k_wgrad_reduce(const float* __restrict__ part, int n_rows, int K,
                                                       float* __restrict__ dW, float* __restrict__ db) {
    __shared__ float sm[32 * 33];
    wgrad_reduce_body<CTW, NH>(blockIdx.x, sm, part, n_rows, K, dW, db);
}

// ---- deferred reductions.  The backward pass leaves every per-block partial (attention-vector and edge-embedding
// partials of each level, the edge-term column sums, the weight-gradient partials) in its own buffer and records a
// task; ONE launch then runs them all (a dependent kernel costs >= 4.6 us of launch-to-launch latency on this
// machine however small it is, and there were 27 of these per step).  (ReduceTask / ReduceTasks: fn_internal.h)
// "fat" bodies for the task-table kernel: a block reduces 32 columns of a per-block partial table (32 threads per column:
// column-major [cols][FN_MAX_PART] with contiguous reads, or the engine's row-major rows, rowmajor_sum_32 below), or a
// 1024-column strip of the row-major weight-gradient partials (wgrad_reduce_strip) -- ~1.5 k blocks per backward pass
// instead of ~10 k one-column blocks.
// the same sum with 32 threads per column (a 1024-thread block takes 32 columns: a quarter of the blocks of the 128-thread form --
// the deferred-reduction launch is mostly block scheduling, §6); no LDS, no barrier: the half-wave's butterfly finishes it
__device__ __forceinline__ float colmajor_sum_32(const float* __restrict__ col, int n_rows) {
    const int lane = threadIdx.x & 31;
    float v = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    int r = lane;
    for (; r + 96 < n_rows; r += 128) { v += col[r];  v1 += col[r + 32];  v2 += col[r + 64];  v3 += col[r + 96]; }
    for (; r < n_rows; r += 32) v += col[r];
    v = (v + v1) + (v2 + v3);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// The row-major twin (the engine's tables, part_at in fn_internal.h): the 32 columns [col0, col0 + 32) of part [n_rows][ld] by one
// 1024-thread block, the sum of column col0 + (threadIdx.x >> 5) returned to all 32 threads of that half-wave.  The ADDITIONS are
// colmajor_sum_32's, operand for operand -- every gradient keeps its bits -- only the threads that do them differ: the four chains of
// lane r of a column run in thread 32 r + c (c: the column), so a wave reads two rows x 32 consecutive columns (128-byte runs; the
// stride-ld walk of one column by one half-wave would be 32 sectors per load); the chain sums then change threads through LDS
// (sm: 32 x 33 floats) to the half-wave that owns the column, which joins them with the very same butterfly.
__device__ __forceinline__ float rowmajor_sum_32(const float* __restrict__ part, int ld, int col0, int n_rows, float* sm) {
    const int c = threadIdx.x & 31, lane = threadIdx.x >> 5;
    const float* __restrict__ p = part + col0 + c;
    float v = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    int r = lane;
    for (; r + 96 < n_rows; r += 128) {
        v += p[(size_t)r * ld];  v1 += p[(size_t)(r + 32) * ld];  v2 += p[(size_t)(r + 64) * ld];  v3 += p[(size_t)(r + 96) * ld];
    }
    for (; r < n_rows; r += 32) v += p[(size_t)r * ld];
    v = (v + v1) + (v2 + v3);
    sm[lane * 33 + c] = v;
    __syncthreads();
    v = sm[(threadIdx.x & 31) * 33 + (threadIdx.x >> 5)];       // lane threadIdx.x & 31 of column threadIdx.x >> 5
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <int CTW, int NH, bool PLAIN = false>
__device__ __forceinline__ void wgrad_reduce_strip(int vb, float* sm, const float* __restrict__ part, int n_rows, int K,
                                                   float* __restrict__ dW, float* __restrict__ db) {
    // a block sums a 1024-column strip of the partial rows: 256 float4 columns x 4 row groups (4 KiB contiguous per wave and
    // row), four loads per thread in flight.  (Round 3: a strip used to be 256 columns x 16 row groups -- 65 blocks of 16
    // waves per product that loaded two float4 each; a quarter of the waves now.)
    constexpr int XW = 16 * CTW * NH;
    constexpr int PW = 128 * XW + 128;
    const int c4 = threadIdx.x & 255, rg = threadIdx.x >> 8;
    const int col0 = vb * 1024 + c4 * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (col0 < PW) {
        float4 a1 = acc, a2 = acc, a3 = acc;
        int r = rg;
        for (; r + 12 < n_rows; r += 16) {
            const float4 v0 = ld4(part + (size_t)r * PW + col0), v1 = ld4(part + (size_t)(r + 4) * PW + col0);
            const float4 v2 = ld4(part + (size_t)(r + 8) * PW + col0), v3 = ld4(part + (size_t)(r + 12) * PW + col0);
            acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
            a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
            a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
            a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
        }
        for (; r < n_rows; r += 4) {
            const float4 v = ld4(part + (size_t)r * PW + col0);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        acc.x = (acc.x + a1.x) + (a2.x + a3.x);  acc.y = (acc.y + a1.y) + (a2.y + a3.y);
        acc.z = (acc.z + a1.z) + (a2.z + a3.z);  acc.w = (acc.w + a1.w) + (a2.w + a3.w);
    }
    st4(sm + rg * 1024 + c4 * 4, acc);
    __syncthreads();
    const int col = vb * 1024 + threadIdx.x;
    if (col < PW) {
        const float v = (sm[threadIdx.x] + sm[1024 + threadIdx.x]) + (sm[2048 + threadIdx.x] + sm[3072 + threadIdx.x]);
        if (col >= 128 * XW) {
            db[col - 128 * XW] = v;
        } else if (PLAIN) {                                                          // k_wgrad128_multi: partials are [o][k] already
            dW[col] = v;
        } else {
            const int r = col & 3, lane = (col >> 2) & 63, tile = col >> 8;        // tile = (w*2+u)*CTW + cc
            const int cc = tile % CTW, wu = tile / CTW, u = wu & 1, w = wu >> 1;
            const int o = 32 * (w & 3) + 16 * u + 4 * (lane >> 4) + r;
            const int xc = 16 * (CTW * (w >> 2) + cc) + (lane & 15);
            if (xc < K) dW[(size_t)o * K + xc] = v;
        }
    }
}

// dL/d(attention vector, edge embedding) of a two-pass or one-pass attention level from the partials its passes wrote.
// blocks 0..255: one column each of the column-major [256][FN_MAX_PART] a_dst/a_src partials; block 256 (mode 2
// only): the [n_e, H*(K+1)] edge-embedding partials and the chain rule through the folded weights.
// (body shared by k_gat_finalize and the deferred task-table kernel k_reduce_tasks; vb = virtual block index,
// sm = 1200 floats of shared memory)
__device__ __forceinline__ void gat_finalize_body(int vb, float* sm, const float* __restrict__ part_a, int n_a,
                                                  const float* __restrict__ part_e, int n_e, const fn_edge_term& et,
                                                  const float* __restrict__ att, int att_w, int dst_off, int src_off,
                                                  float* __restrict__ g_att, float* __restrict__ g_embW,
                                                  float* __restrict__ g_embb, int H) {
    float* s16 = sm;
    float(*redE)[128] = reinterpret_cast<float(*)[128]>(sm + 16);
    float* sE = sm + 16 + 1024;
    const int tid = threadIdx.x;
    if (vb < 2 * FN_D) {
        const int col = vb;
        float mine = 0.f;
        for (int r = tid; r < n_a; r += 1024) mine += part_a[(size_t)col * FN_MAX_PART + r];
        const float v = block_sum_1024(mine, s16);
        if (tid == 0) {
            const int DH = FN_D / H;
            const int cc = col & 127, part = col >> 7;
            g_att[(cc / DH) * att_w + (part ? src_off : dst_off) + (cc % DH)] = v;
        }
        return;
    }
    const int K = et.K, d_e = et.d_e;
    const int ne = H * (K + 1);     // <= 72
    {   // column sums of part_e [n_e][ne]: the 1024 threads form (1024 / cp) row groups x cp columns, cp = pow2 >= ne
        float* red = &redE[0][0];   // 1024 floats
        int cp = 8;
        while (cp < ne) cp <<= 1;
        const int groups = 1024 / cp, col = tid % cp, grp = tid / cp;
        float acc = 0.f;
        if (col < ne) {
            // four loads in flight per thread: with one, this single block was a chain of ~30 dependent round trips (n_e =
            // 3888 partial rows for the bond level) and the whole deferred-reduction launch waited for it (25 -> 14 us)
            float a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int r = grp;
            for (; r + 3 * groups < n_e; r += 4 * groups) {
                acc += part_e[(size_t)r * ne + col];
                a1 += part_e[(size_t)(r + groups) * ne + col];
                a2 += part_e[(size_t)(r + 2 * groups) * ne + col];
                a3 += part_e[(size_t)(r + 3 * groups) * ne + col];
            }
            for (; r < n_e; r += groups) acc += part_e[(size_t)r * ne + col];
            acc = (acc + a1) + (a2 + a3);
        }
        red[grp * cp + col] = acc;
        __syncthreads();
        if (tid < 128) {
            float v = 0.f;
            if (tid < ne)
                for (int g = 0; g < groups; ++g) v += red[g * cp + tid];
            sE[tid] = v;
        }
        __syncthreads();
    }
    if (tid < H * d_e) {
        const int hh = tid / d_e, c = tid % d_e;
        float a = sE[hh * (K + 1) + K] * et.embb[c];
        for (int k = 0; k < K; ++k) a = fmaf(sE[hh * (K + 1) + k], et.embW[c * K + k], a);
        g_att[hh * att_w + et.mid_off + c] = a;
    }
    if (tid < d_e * K) {
        const int c = tid / K, k = tid % K;
        float a = 0.f;
        for (int hh = 0; hh < H; ++hh) a = fmaf(sE[hh * (K + 1) + k], att[hh * att_w + et.mid_off + c], a);
        g_embW[tid] = a;
    }
    if (tid < d_e) {
        float a = 0.f;
        for (int hh = 0; hh < H; ++hh) a = fmaf(sE[hh * (K + 1) + K], att[hh * att_w + et.mid_off + tid], a);
        g_embb[tid] = a;
    }
}

// the stand-alone launch of gat_finalize_body (fn_gat_bwd_finalize_f32): beside the task-table kernel that runs the same body
__global__ __launch_bounds__(1024) void k_gat_finalize(const float* __restrict__ part_a, int n_a,
                                                       const float* __restrict__ part_e, int n_e, fn_edge_term et,
                                                       const float* __restrict__ att, int att_w, int dst_off,
                                                       int src_off, float* __restrict__ g_att,
                                                       float* __restrict__ g_embW, float* __restrict__ g_embb, int H) {
    __shared__ float sm[1200];
    gat_finalize_body(blockIdx.x, sm, part_a, n_a, part_e, n_e, et, att, att_w, dst_off, src_off, g_att, g_embW, g_embb, H);
}

__global__ __launch_bounds__(1024) void k_reduce_tasks(ReduceTasks T, AdamRide R) {
    __shared__ float sm[16 * 256];
    if (R.nblk && (int)blockIdx.x >= R.first) { adam_ride(R);  return; }
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.first[ti + 1]) ++ti;
    const ReduceTask& t = T.t[ti];
    const int vb = (int)blockIdx.x - T.first[ti];
    if (t.kind == RT_FINALIZE) {
        if (vb < 2 * FN_D / 32) {
            const int col = vb * 32 + (threadIdx.x >> 5);
            const float v = t.pld ? rowmajor_sum_32(t.p0, t.pld, vb * 32, t.n0, sm) : colmajor_sum_32(t.p0 + (size_t)col * FN_MAX_PART, t.n0);
            if ((threadIdx.x & 31) == 0) {
                const int DH = FN_D / t.H, cc = col & 127, part = col >> 7;
                t.o0[(cc / DH) * t.att_w + (part ? t.src_off : t.dst_off) + (cc % DH)] = v;
            }
        } else {             // (the one block behind them: a level with an embedded edge attribute, mode 2)
            gat_finalize_body(2 * FN_D, sm, t.p0, t.n0, t.p1, t.n1, t.et, t.att, t.att_w, t.dst_off, t.src_off, t.o0, t.o1, t.o2, t.H);
        }
    } else if (t.kind == RT_COLSUM) {
        const int col = vb * 32 + (threadIdx.x >> 5);
        const float v = t.pld ? rowmajor_sum_32(t.p0, t.pld, vb * 32, t.n0, sm) : colmajor_sum_32(t.p0 + (size_t)col * FN_MAX_PART, t.n0);
        if ((threadIdx.x & 31) == 0) t.o0[(col / FN_D) * t.ld + t.off + (col % FN_D)] = v;
    } else {
        switch (t.cls) {      // ReduceTask::cls: the class of the kernel that wrote the partials (wgrad_class, below)
            case 0: wgrad_reduce_strip<1, 1>(vb, sm, t.p0, t.n0, t.K, t.o0, t.o1); break;
            case 1: wgrad_reduce_strip<1, 2>(vb, sm, t.p0, t.n0, t.K, t.o0, t.o1); break;
            case 2: wgrad_reduce_strip<4, 2>(vb, sm, t.p0, t.n0, t.K, t.o0, t.o1); break;
            case 4: wgrad_reduce_strip<4, 2, true>(vb, sm, t.p0, t.n0, t.K, t.o0, t.o1); break;
            default: wgrad_reduce_strip<6, 2>(vb, sm, t.p0, t.n0, t.K, t.o0, t.o1); break;
        }
    }
}

// ---- the K class: which instance <CTW, NH> of the partial-product kernels (wgrad_body) and of the reductions (wgrad_reduce_body /
// wgrad_reduce_strip) serves a reduction length K.  Decided HERE for every host path; the value is ReduceTask::cls, which the switch of
// k_reduce_tasks reads (its `default` is class 3).
//   class 0: K <= 16  <1, 1>     class 1: K <= 32  <1, 2>     class 2: K <= 128  <4, 2>     class 3: K <= 192  <6, 2>
//   class 4: the direct K = 128 kernel (wgrad128.inc): partials of class 2's width in plain [o][k] layout; never returned from here
// mixed: the grouped layer-0 launch (k_linear128_wgrad_mixed, k_wgrad_all) has 512-thread instances only: it runs K <= 16 in class 1
constexpr int kWgCtw[5] = {1, 1, 4, 6, 4}, kWgNh[5] = {1, 2, 2, 2, 2};
constexpr int kWgClassDirect128 = 4;
inline int wgrad_class(int K, bool mixed = false) { return K <= 16 ? (mixed ? 1 : 0) : K <= 32 ? 1 : K <= 128 ? 2 : K <= 192 ? 3 : -1; }
inline int wgrad_class_xw(int cls) { return 16 * kWgCtw[cls] * kWgNh[cls]; }                  // padded X width the class holds in LDS
inline int64_t wgrad_class_width(int cls) { return (int64_t)128 * wgrad_class_xw(cls) + 128; }       // floats of one partial row
inline size_t wgrad_class_lds(int cls) { return (size_t)2 * kWgChunk * (kBtLd + wgrad_class_xw(cls) + 16) * sizeof(float); }

template <int CTW, int NH>
int launch_wgrad(const float* dY, const float* X, int K, int64_t M, int rpb, int grid, float* part, float* dW, float* db,
                 hipStream_t st) {
    constexpr int XW = 16 * CTW * NH, XLD = XW + 16, PW = 128 * XW + 128;
    const size_t lds = (size_t)2 * kWgChunk * (kBtLd + XLD) * sizeof(float);
    if (int rc = allow_lds(k_linear128_wgrad<CTW, NH>, lds)) return rc;
    hipLaunchKernelGGL((k_linear128_wgrad<CTW, NH>), dim3(grid), dim3(256 * NH), lds, st, dY, X, K, M, rpb, part);
    if (dW) hipLaunchKernelGGL((k_wgrad_reduce<CTW, NH>), dim3((PW + 31) / 32), dim3(1024), 0, st, part, grid, K, dW, db);
    return 0;
}
// ... of class cls (0..3)
int launch_wgrad_class(int cls, const float* dY, const float* X, int K, int64_t M, int rpb, int grid, float* part, float* dW, float* db,
                       hipStream_t st) {
    int rc = 0;
    with_const<0, 1, 2, 3>(cls, [&](auto c) { rc = launch_wgrad<kWgCtw[FN_CV(c)], kWgNh[FN_CV(c)]>(dY, X, K, M, rpb, grid, part, dW, db, st); });
    return rc;
}
// (a K beyond every class: the widest class's width, as the workspace size of such a K always was)
inline int64_t wgrad_part_width(int K) { return wgrad_class_width(K <= 192 ? wgrad_class(K) : 3); }
inline int wgrad_rows_per_block(int64_t M) {
    int64_t rpb = (M + 255) / 256;
    rpb = (rpb + kWgChunk - 1) / kWgChunk * kWgChunk;
    return (int)(rpb < kWgChunk ? kWgChunk : rpb);
}

// weight-gradient partials only (the reduction is deferred); *grid = partial rows written, *cls = kernel class
int wgrad_partials(const float* dY, const float* X, int K, int64_t M, float* ws, hipStream_t st, int* grid, int* cls) {
    const int rpb = wgrad_rows_per_block(M);
    *grid = (int)((M + rpb - 1) / rpb);
    *cls = wgrad_class(K);
    if (*cls < 0) return fail(FN_EUNSUPPORTED, "weight gradient: K > 192");
    return launch_wgrad_class(*cls, dY, X, K, M, rpb, *grid, ws, nullptr, nullptr, st);
}

}  // namespace

// =====================================================================================
// fni::ParamGradQueue (fn_internal.h): the deferred parameter work of one backward pass
// =====================================================================================
namespace fni {

int ParamGradQueue::flush(bool last) {
    if (int rc = flush_wgrad()) return rc;
    const AdamRide R = make_adam_ride(last ? rider : nullptr, blocks, 1024, tune(FN_TUNE_RIDER_PIECES));
    if (T.n == 0 && R.nblk == 0) return 0;
    hipLaunchKernelGGL(k_reduce_tasks, dim3(blocks + R.nblk), dim3(1024), 0, st, T, R);
    T.n = 0;  blocks = 0;
    const int rc = launch_status("deferred reductions");
    if (rc == 0 && R.nblk > 0) rider->launched = 1;      // the caller's Adam launch may now skip the slice (fn_adam_slice.launched)
    return rc;
}
int ParamGradQueue::push(ReduceTask t, int nblk) {
    if (T.n == kMaxReduceTasks) { if (int rc = flush()) return rc; }
    t.first = blocks;  t.nblk = nblk;
    T.first[T.n] = blocks;
    T.t[T.n++] = t;
    blocks += nblk;
    return 0;
}
int ParamGradQueue::finalize(const AttParamGrads& a) {
    ReduceTask t{};
    t.kind = RT_FINALIZE;  t.H = a.H;  t.p0 = a.part_a;  t.n0 = a.n_a;  t.p1 = a.part_e;  t.n1 = a.n_e;  t.et = a.et;
    t.att = a.att;  t.att_w = a.att_w;  t.dst_off = 0;  t.src_off = a.src_off;  t.o0 = a.g_att;  t.o1 = a.g_embW;  t.o2 = a.g_embb;
    t.pld = a.part_ld;
    return push(t, 2 * FN_D / 32 + (a.et.mode == 2 ? 1 : 0));
}
int ParamGradQueue::colsum(const float* part, int n_rows, int cols, float* out, int ld, int off, int part_ld) {
    ReduceTask t{};
    t.kind = RT_COLSUM;  t.p0 = part;  t.n0 = n_rows;  t.o0 = out;  t.ld = ld;  t.off = off;  t.pld = part_ld;
    if (cols % 32) return fail(FN_EINVAL, "deferred column sum: column count must be a multiple of 32");
    return push(t, cols / 32);
}
int ParamGradQueue::wgrad(const ProjWgrad& p, hipStream_t launch_on) {
    const int K = p.K;
    const int64_t M = p.M;
    float* ws = p.ws;
    if (M == 0) {
        hipLaunchKernelGGL(k_zero2_i32, dim3(flat_grid(128 * (K + 1), kGridCap)), dim3(kBlock), 0, launch_on,
                           reinterpret_cast<int32_t*>(p.dW), (int64_t)128 * K, reinterpret_cast<int32_t*>(p.db), (int64_t)128);
        return launch_status("weight gradient (empty)");
    }
    ReduceTask t{};
    int grid = 0;
    if (K == FN_D) {   // partial product joins the grouped launch in flush(); its block count is set there
        if (W.n == kMaxWgradTasks || T.n == kMaxReduceTasks) { if (int rc = flush()) return rc; }
        W.t[W.n] = WgradTask{p.g_h, p.x, ws, M, 0, 0, 0, p.n_real};
        w_reduce[W.n++] = T.n;
        t.cls = tune(FN_TUNE_WGRAD_DIRECT) ? kWgClassDirect128 : wgrad_class(FN_D);
    } else if (defer_mixed && K <= 192) {      // layer 0's products: one launch for them too (flush_wgrad)
        if (W0.n == kMaxWgradTasks || T.n == kMaxReduceTasks) { if (int rc = flush()) return rc; }
        // rows per block: a multiple of the per-product rule (FN_TUNE_WGRAD0_ROWS).  Fewer, longer blocks = fewer partial
        // rows to write and to reduce: at 1 x layer 0's atom product alone wrote 217 partials of 98 KB (21 MB, more than the
        // nine K = 128 products together).  2 x for it, 3 x for the narrow ones: -6 us per step; 3 x / 4 x for the wide one
        // or 1 x for it lose (the long blocks become the launch's tail / the partial traffic is back)
        const int tv = tune(FN_TUNE_WGRAD0_ROWS) > 0 ? tune(FN_TUNE_WGRAD0_ROWS) : 23;
        const int mult = std::max(1, K > FN_D ? tv / 10 : tv % 10);          // tens: the wide product (atoms), units: the narrow ones
        const int rpb = wgrad_rows_per_block(M) * mult;
        grid = (int)((M + rpb - 1) / rpb);
        W0.t[W0.n++] = WgradTask{p.g_h, p.x, ws, M, rpb, w0blocks, K, p.n_real};
        w0blocks += grid;
        t.cls = wgrad_class(K, true);
    } else if (int rc = wgrad_partials(p.g_h, p.x, K, M, ws, launch_on, &grid, &t.cls)) return rc;
    t.kind = RT_WGRAD;  t.p0 = ws;  t.n0 = grid;  t.K = K;  t.o0 = p.dW;  t.o1 = p.db;
    return push(t, (int)((wgrad_class_width(t.cls) + 1023) / 1024));      // 1024-column strips of the class's partial rows
}
// block counts of the K = 128 group.  Rows per block from the WHOLE group: ~256 blocks (one per CU) instead of ~256 per product,
// which for the nine products of a backward pass was 1.6 k blocks writing 104 MB of 64-KB partials (now ~16 MB); never fewer rows
// than the per-product rule, so the partial workspace sized by fn_linear128_wgrad_ws still fits
void ParamGradQueue::size_group128() {
    int64_t total = 0;
    for (int i = 0; i < W.n; ++i) total += W.t[i].M;
    const int64_t target = tune(FN_TUNE_WGRAD_BLOCKS) > 0 ? tune(FN_TUNE_WGRAD_BLOCKS) : 256;
    const int group_rpb = (int)(((total + target - 1) / target + kWgChunk - 1) / kWgChunk * kWgChunk);
    wblocks = 0;
    for (int i = 0; i < W.n; ++i) {
        WgradTask& t = W.t[i];
        t.rpb = std::max(group_rpb, wgrad_rows_per_block(t.M));
        t.first = wblocks;
        const int grid = (int)((t.M + t.rpb - 1) / t.rpb);
        T.t[w_reduce[i]].n0 = grid;
        wblocks += grid;
    }
    W.K = FN_D;
}
int ParamGradQueue::flush_wgrad() {
    size_t lds0 = 0;
    if (W0.n) {      // the largest product's class
        int kmax = 0;
        for (int i = 0; i < W0.n; ++i) kmax = std::max(kmax, W0.t[i].K);
        lds0 = wgrad_class_lds(wgrad_class(kmax, true));
    }
    if (W0.n && W.n && tune(FN_TUNE_WGRAD_DIRECT) == 1 && tune(FN_TUNE_GEMM_COLAUNCH) != 0) {
        size_group128();         // both groups in one launch (k_wgrad_all)
        const size_t lds = std::max(lds0, (size_t)wd_lds_bytes<2>());
        if (int rc = allow_lds(k_wgrad_all, lds)) return rc;
        hipLaunchKernelGGL(k_wgrad_all, dim3(wblocks + w0blocks), dim3(512), lds, st, W, W0, wblocks);
        W.n = 0;  wblocks = 0;  W0.n = 0;  w0blocks = 0;
        return launch_status("weight-gradient partials (all products)");
    }
    if (W0.n) {
        const size_t lds = lds0;
        if (int rc = allow_lds(k_linear128_wgrad_mixed, lds)) return rc;
        hipLaunchKernelGGL(k_linear128_wgrad_mixed, dim3(w0blocks), dim3(512), lds, st, W0);
        W0.n = 0;  w0blocks = 0;
        if (int rc = launch_status("weight-gradient partials (layer 0)")) return rc;
    }
    if (W.n == 0) return 0;
    size_group128();
    if (tune(FN_TUNE_WGRAD_DIRECT)) {
        if (int rc = allow_lds(k_wgrad128_multi<2>, wd_lds_bytes<2>())) return rc;
        hipLaunchKernelGGL(k_wgrad128_multi<2>, dim3(wblocks), dim3(wd_threads<2>()), wd_lds_bytes<2>(), st, W);
    } else {
        const size_t lds = wgrad_class_lds(wgrad_class(FN_D));
        if (int rc = allow_lds(k_linear128_wgrad_multi<4, 2>, lds)) return rc;
        hipLaunchKernelGGL((k_linear128_wgrad_multi<4, 2>), dim3(wblocks), dim3(512), lds, st, W);
    }
    W.n = 0;  wblocks = 0;
    return launch_status("grouped weight-gradient partials");
}

}  // namespace fni

// ---- the operator entry points of the family
extern "C" {

int fn_gat_bwd_finalize_f32(const float* part_a, int n_part_a, const float* part_e, int n_part_e, const fn_edge_term* et,
                            const float* att, int att_w, int dst_off, int src_off, float* g_att, float* g_embW,
                            float* g_embb, int heads, fn_stream_t stream) {
    if (!part_a || n_part_a < 0 || n_part_e < 0 || !att || !g_att || fni::bad_edge_term(et, 0)) return fail(FN_EINVAL, "fn_gat_bwd_finalize_f32: bad argument");
    if (et->mode == 2 && (!part_e || !g_embW || !g_embb)) return fail(FN_EINVAL, "fn_gat_bwd_finalize_f32: null mode-2 buffer");
    if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return fail(FN_EUNSUPPORTED, "heads must be 1, 2, 4 or 8");
    hipLaunchKernelGGL(k_gat_finalize, dim3(2 * FN_D + (et->mode == 2 ? 1 : 0)), dim3(1024), 0, S(stream), part_a, n_part_a, part_e, n_part_e, *et, att,
                       att_w, dst_off, src_off, g_att, g_embW, g_embb, heads);
    return launch_status("fn_gat_bwd_finalize_f32");
}

int64_t fn_linear128_wgrad_ws(int64_t M, int K) {
    const int rpb = wgrad_rows_per_block(M);
    const int64_t grid = (M + rpb - 1) / rpb;
    return (grid < 1 ? 1 : grid) * wgrad_part_width(K);
}

int fn_linear128_wgrad_f32(const float* dY, const float* X, int K, int64_t M, float* ws, float* dW, float* db, fn_stream_t stream) {
    if (K < 1 || M < 0 || !dW || !db) return fail(FN_EINVAL, "fn_linear128_wgrad_f32: bad argument");
    if (M == 0) {
        hipLaunchKernelGGL(k_zero2_i32, dim3(flat_grid(128 * (K + 1), kGridCap)), dim3(kBlock), 0, S(stream),
                           reinterpret_cast<int32_t*>(dW), (int64_t)128 * K, reinterpret_cast<int32_t*>(db), (int64_t)128);
        return launch_status("fn_linear128_wgrad_f32");
    }
    if (!dY || !X || !ws || ((uintptr_t)dY & 15)) return fail(FN_EINVAL, "fn_linear128_wgrad_f32: null or misaligned buffer");
    const int rpb = wgrad_rows_per_block(M);
    const int grid = (int)((M + rpb - 1) / rpb);
    const int cls = wgrad_class(K);
    if (cls < 0) return fail(FN_EUNSUPPORTED, "fn_linear128_wgrad_f32: K > 192");
    if (int rc = launch_wgrad_class(cls, dY, X, K, M, rpb, grid, ws, dW, db, S(stream))) return rc;
    return launch_status("fn_linear128_wgrad_f32");
}

}  // extern "C"
