// input_grad.hip -- the gradient of layer 0's three projections with respect to their INPUTS (reference gat2.py:138, 186, 241:
// projection_b / projection_a / projection_fb applied to the raw bond, atom and fragment-connection feature tables).  A translation
// unit of its own: no existing kernel instance changes.
//   dx[m, k]  = sum_j g[m, j] W[j, k]           g [M, 128] = dL/d(projection output), W [128, K] = nn.Linear's weight as stored, 1 <= K <= 168
//   dots[m]   = sum_k dx[m, k] delta[m, k]      (optional: gradient x input, or integrated gradients' (x - x0) . grad, without dx in memory)
// Up to three such tasks share one launch (task table, as tower.hip / attn_readout.hip).  The output width is ragged: a dx row is K
// floats, element-aligned only, nothing is padded in memory; the last, partial 16-column tile masks its loads and its stores.
//
// A workgroup = 4 waves; it stages its task's W in LDS once ([128][LD], LD = 16 NT + 4 with NT = ceil(K / 16) column tiles, the padding
// columns zero) and walks 64-row tiles, wave w the rows [64 t + 16 w, + 16).  A lane (n, q) = (l & 15, l >> 4) reads its row's g once,
// as eight 16-byte pieces g[row n][16 i + 4 q .. + 3]; MFMA step (i, c) pairs j = 16 i + 4 q + c of both operands, so the B operand is
// W_lds[(16 i + 4 q + c) LD + 16 ct + n]: the four quarters of a wave hit four different groups of 16 banks (4 LD = 16 mod 64).  One
// accumulator per column tile, the 32 steps of j in a fixed order: every output element is the same sum in every run.
// dots: the products dx * delta of a wave's 16 rows go to an LDS tile ([16][16 NT + 1]); one lane per row then adds its row's K products in
// ASCENDING k.  No atomics, nothing depends on the grid.
// Arithmetic: fp32 in, fp32 accumulate, v_mfma_f32_16x16x4_f32 only.
#include <stdint.h>

#include <algorithm>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

constexpr int kDxMaxK = 168;
constexpr int kDxWaves = 4;                                        // waves per workgroup = 16-row tiles per step
constexpr int kDxMaxBlocks = 512;                                  // per task; a block with more than one tile strides over them

struct DxTasks {
    fn_linear_dx_task t[FN_MAX_DX_TASKS];
    int first[FN_MAX_DX_TASKS], nblk[FN_MAX_DX_TASKS];
    int n;
};
inline int dx_tiles(int K) { return (K + 15) / 16; }
inline int dx_ld(int K) { return 16 * dx_tiles(K) + 4; }           // W's LDS row stride (floats)
inline int dx_ldp(int K) { return 16 * dx_tiles(K) + 1; }          // the product tile's
inline size_t dx_lds_floats(int K, bool dots) { return (size_t)FN_D * dx_ld(K) + (dots ? (size_t)kDxWaves * 16 * dx_ldp(K) : 0); }

__global__ __launch_bounds__(64 * kDxWaves) void k_linear_dx(const DxTasks T) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, l = tid & 63, n = l & 15, q = l >> 4, wv = tid >> 6;
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.first[ti + 1]) ++ti;
    const fn_linear_dx_task& t = T.t[ti];
    const int blk = (int)blockIdx.x - T.first[ti], nblk = T.nblk[ti];
    const int K = t.K, NT = (K + 15) >> 4, LD = 16 * NT + 4, LDP = 16 * NT + 1;
    const int64_t M = t.M;
    float* Ws = sm;                                                // [128][LD]
    float* Ps = sm + FN_D * LD + wv * 16 * LDP;                    // this wave's [16][LDP] (tasks with dots only)
    const float* __restrict__ W = t.W;
    const float* __restrict__ g = t.g;
    const float* __restrict__ delta = t.delta;
    float* __restrict__ dx = t.dx;
    float* __restrict__ dots = t.dots;

    for (int i = tid; i < FN_D * LD; i += 64 * kDxWaves) {         // W -> LDS; columns K .. LD - 1 are zero
        const int j = i / LD, c = i - j * LD;
        Ws[i] = c < K ? W[j * K + c] : 0.f;
    }
    const int64_t tiles = (M + 16 * kDxWaves - 1) / (16 * kDxWaves);
    for (int64_t tile = blk; tile < tiles; tile += nblk) {         // (the trip count is the workgroup's: the barriers below are uniform)
        const int64_t r0 = tile * (16 * kDxWaves) + 16 * wv;
        float4 a[8];
        {
            const int64_t r = r0 + n;
            const float* gp = g + (size_t)(r < M ? r : 0) * FN_D + 4 * q;
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = r < M ? ld4(gp + 16 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();                                           // W staged / the previous tile's products are read
        for (int ct = 0; ct < NT; ++ct) {
            const float* wp = Ws + (4 * q) * LD + 16 * ct + n;
            float b[32];                                           // the tile's 32 B operands first, then the MFMA chain
#pragma unroll
            for (int i = 0; i < 8; ++i) {
#pragma unroll
                for (int c = 0; c < 4; ++c) b[4 * i + c] = wp[(16 * i + c) * LD];
            }
            __builtin_amdgcn_sched_barrier(0);                     // (the scheduler otherwise sinks every read to its MFMA: read, wait, multiply, 32 times)
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                DN_MFMA(acc, a[i].x, b[4 * i + 0]);
                DN_MFMA(acc, a[i].y, b[4 * i + 1]);
                DN_MFMA(acc, a[i].z, b[4 * i + 2]);
                DN_MFMA(acc, a[i].w, b[4 * i + 3]);
            }
            // acc[e] = (row r0 + 4 q + e, column 16 ct + n)
            const int col = 16 * ct + n;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t r = r0 + 4 * q + e;
                const bool ok = r < M && col < K;
                if (dx && ok) dx[(size_t)r * K + col] = acc[e];
                if (dots) Ps[(4 * q + e) * LDP + col] = ok ? acc[e] * delta[(size_t)r * K + col] : 0.f;
            }
        }
        if (dots) {
            __syncthreads();
            if (l < 16 && r0 + l < M) {
                const float* pr = Ps + l * LDP;
                float s = 0.f;
                for (int k = 0; k < K; ++k) s += pr[k];
                dots[r0 + l] = s;
            }
        }
    }
}
}  // namespace

namespace fni {
int launch_linear_dx(const fn_linear_dx_task* tasks, int n_tasks, hipStream_t st) {
    if (!tasks || n_tasks < 1 || n_tasks > FN_MAX_DX_TASKS) return fail(FN_EINVAL, "fn_linear_dx_f32: 1 .. FN_MAX_DX_TASKS tasks");
    DxTasks T{};
    int blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < n_tasks; ++i) {
        const fn_linear_dx_task& t = tasks[i];
        if (t.K < 1 || t.K > kDxMaxK) return fail(FN_EUNSUPPORTED, "fn_linear_dx_f32: K must be in [1, 168]");
        if (t.M < 0) return fail(FN_EINVAL, "fn_linear_dx_f32: negative row count");
        if (t.M == 0 || (!t.dx && !t.dots)) continue;              // nothing to write
        if (!t.g || !t.W || (t.dots && !t.delta)) return fail(FN_EINVAL, "fn_linear_dx_f32: null g / W, or dots without delta");
        if (misaligned(15, t.g) || misaligned(3, t.W, t.dx, t.delta, t.dots)) return fail(FN_EINVAL, "fn_linear_dx_f32: g must be 16-byte aligned, the rest element-aligned");
        const int64_t tiles = (t.M + 16 * kDxWaves - 1) / (16 * kDxWaves);
        T.t[T.n] = t;
        T.first[T.n] = blocks;
        T.nblk[T.n] = (int)(tiles < kDxMaxBlocks ? tiles : kDxMaxBlocks);
        blocks += T.nblk[T.n];
        lds = std::max(lds, dx_lds_floats(t.K, t.dots != nullptr) * sizeof(float));
        ++T.n;
    }
    if (!T.n) return 0;
    static bool once = false;                                      // (the widest task with dots: 134 KB of the CU's 160)
    if (!once) { FN_TRY(allow_lds(k_linear_dx, dx_lds_floats(kDxMaxK, true) * sizeof(float)));  once = true; }
    hipLaunchKernelGGL(k_linear_dx, dim3(blocks), dim3(64 * kDxWaves), lds, st, T);
    return launch_status("fn_linear_dx_f32");
}
}  // namespace fni

extern "C" {

int fn_linear_dx_f32(const fn_linear_dx_task* tasks, int n_tasks, fn_stream_t stream) { return fni::launch_linear_dx(tasks, n_tasks, S(stream)); }

}  // extern "C"
