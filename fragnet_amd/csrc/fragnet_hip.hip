// libfragnet_hip.so -- gfx950 (MI355X / CDNA4) kernels for FragNet's four-level message passing.
// C-ABI declared in include/fragnet_hip.h (which cites the reference call sites replaced).
// This unit is the OPERATOR SURFACE -- what ops.py calls one operator at a time: segment sum / softmax, gathers, row dots, dropout, losses,
// Adam, the projection launches (fn_linear128_f32 and the grouped forms), the destination pass of the two-pass attention backward -- and the home of the
// error string, the tuning table and the profiling events (fni::fail / tune / prof_event, fn_internal.h).  The encoder engine is encoder.hip; it also holds the operators whose kernels share a
// device body with one of its combined launches (its header comment lists them).
//
// Layout conventions used by every row kernel below:
//   * node tables are [rows, 128] fp32; one 32-lane half-wavefront owns one row, each lane one
//     float4 (16 B) => a wave64 moves two 512-B rows per load instruction, fully coalesced;
//   * with H heads, head h owns the 32/H consecutive lanes [h*LPH, (h+1)*LPH) of the half-wave, so
//     every per-head reduction is an xor-butterfly over LPH lanes and never leaves the half-wave;
//   * a block is 256 threads = 8 rows; grids are capped and grid-strided so that the number of
//     per-block partial-sum rows any backward kernel writes is bounded by FN_MAX_PART.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fragnet_hip.h"
#include "fn_internal.h"

namespace {

thread_local char tl_err[256] = "";

int fail(int code, const char* what) {
    snprintf(tl_err, sizeof(tl_err), "%s", what);
    return code;
}

int launch_status(const char* where) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(tl_err, sizeof(tl_err), "%s: %s", where, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// (S(), kBlock, kRows, kGridCap, kBwdRows, row_grid, flat_grid, edge_class, lin_blocks, lin_layout, FN_TRY, allow_lds, with_heads: fn_internal.h)
using fni::GatFwdArgs;

// =====================================================================================
// Attention level
// =====================================================================================
#include "gat_fwd.inc"

#include "gat_bwd_two.inc"
#include "shared_bodies.inc"

// =====================================================================================
// Full-width edge term (atom graph / fragment graph), produced directly in destination-sorted order
// =====================================================================================
// s_sorted[pos, j] = <feat[eid(pos), :], A[j, off:off+128]>, 0 at loop positions (eid >= m_real): row_dots_sorted_body (shared_bodies.inc)
__global__ __launch_bounds__(kBlock) void k_row_dots_sorted(const float* __restrict__ feat, const float* __restrict__ A,
                                                            int lda, int off, int J, fn_gat_plan pl,
                                                            float* __restrict__ s_sorted) {
    row_dots_sorted_body<8>(feat, A, lda, off, J, pl, s_sorted, (int)blockIdx.x, (int)gridDim.x);
}

// one block per column of the column-major partials [cols][FN_MAX_PART]
__device__ __forceinline__ void colsum_body(int vb, float* s16, const float* __restrict__ part, int n_rows,
                                            float* __restrict__ out, int ld, int off) {
    const int col = vb;
    float mine = 0.f;
    for (int r = threadIdx.x; r < n_rows; r += 1024) mine += part[(size_t)col * FN_MAX_PART + r];
    const float v = block_sum_1024(mine, s16);
    if (threadIdx.x == 0) out[(col / FN_D) * ld + off + (col % FN_D)] = v;
}
__global__ __launch_bounds__(1024) void k_colsum(const float* __restrict__ part, int n_rows, int cols,
                                                  float* __restrict__ out, int ld, int off) {
    __shared__ float s16[16];
    colsum_body(blockIdx.x, s16, part, n_rows, out, ld, off);
}

// =====================================================================================
// Segment sum / gather / segment softmax (the torch-scatter operator surface)
// =====================================================================================
__global__ __launch_bounds__(kBlock) void k_segment_sum128(const float* __restrict__ src, int64_t src_ld,
                                                           const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ perm, int32_t pos_base,
                                                           float* __restrict__ out, int64_t n_seg) {
    const int lane = threadIdx.x & 31;
    int64_t g0, g1;
    block_groups(n_seg, kRows, g0, g1);
    for (int64_t gi = g0; gi < g1; ++gi) {
        const int64_t s = gi * kRows + (threadIdx.x >> 5);
        if (s >= n_seg) continue;
        const int beg = rowptr[s] - pos_base, deg = rowptr[s + 1] - rowptr[s];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);

        for (int i = 0; i < deg; ++i) {
            const float4 v = ld4(src + (size_t)perm[beg + i] * src_ld + lane * 4);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        st4(out + s * FN_D + lane * 4, acc);
    }
}

// long segments (pooling: ~26 atoms per molecule, few hundred segments): one block per segment, its 8 half-waves
// take rows hw, hw+8, ... and the 8 partial rows are added in a fixed order: block_rows_sum (shared_bodies.inc), which the kernels
// down to k_pool_cat_groups run -- "the same order" between them is one text
__global__ __launch_bounds__(kBlock) void k_segment_sum128_wide(const float* __restrict__ src, int64_t src_ld,
                                                                const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ perm, int32_t pos_base,
                                                                float* __restrict__ out, int64_t n_seg) {
    __shared__ float sS[kRows][FN_D];
    for (int64_t s = blockIdx.x; s < n_seg; s += gridDim.x) {
        block_rows_sum(sS, src, src_ld, perm, rowptr[s] - pos_base, rowptr[s + 1] - rowptr[s], KeepAllRows{},
                       [=](float v) { out[s * FN_D + threadIdx.x] = v; });
        __syncthreads();
    }
}

// pooled = cat(sum of a molecule's atom rows, sum of its fragment rows): [B, 256] in one launch (gat2.py:820-823).
// grid (B, 2): y = 0 atoms -> columns 0..127, y = 1 fragments -> columns 128..255; one block per molecule and half.
// This kernel and its leave-group-out form: choose the segment plan and the table by blockIdx.y, build the predicate, run the body, store.
__global__ __launch_bounds__(kBlock) void k_pool_cat(const float* __restrict__ x_atoms, const float* __restrict__ x_frags,
                                                     fn_seg_plan sa, fn_seg_plan sf, float* __restrict__ out) {
    __shared__ float sS[kRows][FN_D];
    const int64_t r = blockIdx.x, s = r;
    const fn_seg_plan& sp = blockIdx.y ? sf : sa;
    block_rows_sum(sS, blockIdx.y ? x_frags : x_atoms, FN_D, sp.perm, sp.rowptr[s] - sp.pos_base, sp.rowptr[s + 1] - sp.rowptr[s], KeepAllRows{},
                   [=](float v) { out[(size_t)r * 2 * FN_D + blockIdx.y * FN_D + threadIdx.x] = v; });
}
// leave-group-out form of k_pool_cat (fragment contributions, fragnet/vizualize/model_attr.py:186-205: the rows of one fragment are set
// to 0.0 in the encoder's final x_atoms, x_frags stays): output row r is molecule row_mol[r] pooled without the atoms whose group is
// row_group[r].  The same body as k_pool_cat with another predicate; an atom that is left out enters the sum as 0.0, so a row equals
// k_pool_cat's of the same table with those rows overwritten by 0.0, bit for bit, and a row that leaves nothing out equals k_pool_cat's
// row of its molecule.  grid (R, 2) like k_pool_cat's (B, 2).
__global__ __launch_bounds__(kBlock) void k_pool_cat_groups(const float* __restrict__ x_atoms, const float* __restrict__ x_frags,
                                                            fn_seg_plan sa, fn_seg_plan sf, const int64_t* __restrict__ atom_group,
                                                            const int32_t* __restrict__ row_mol, const int64_t* __restrict__ row_group,
                                                            float* __restrict__ out) {
    __shared__ float sS[kRows][FN_D];
    const int64_t r = blockIdx.x, s = row_mol[r];
    const int64_t leave = blockIdx.y ? -1 : row_group[r];      // < 0: nothing is left out (ungrouped atoms carry ids < 0 too)
    const int64_t* grp = leave < 0 ? nullptr : atom_group;     // null: nothing is left out, and atom_group is not read for a fragment row
    const auto keep = [=](int32_t row) { return !grp || grp[row] != leave; };
    const fn_seg_plan& sp = blockIdx.y ? sf : sa;
    block_rows_sum(sS, blockIdx.y ? x_frags : x_atoms, FN_D, sp.perm, sp.rowptr[s] - sp.pos_base, sp.rowptr[s + 1] - sp.rowptr[s], keep,
                   [=](float v) { out[(size_t)r * 2 * FN_D + blockIdx.y * FN_D + threadIdx.x] = v; });
}
// coalition form of k_pool_cat (fragment Shapley values): output row r is molecule row_mol[r] pooled over the atoms that are in no group
// (atom_bit < 0) or whose bit atom_bit[i] of row_mask[r] is set; the fragments' half is never masked.
// The simple form: one workgroup per row and half, grid (R, 2) -- the yardstick of the tiled form below (FN_TUNE_COALITION_STAGED).
// The body is written out here and reproduces block_rows_sum's partition and order with k_pool_cat_groups' treatment of a left-out atom
// (0.0, load skipped), so the same bit-for-bit statements hold (tests/test_gpu_pool_sums.py holds it to them).  As a wrapper of
// block_rows_sum this kernel waited for row_mask[r] in front of the item loop and its launches took 5 to 11 % longer
// (profiles/pool_bodies_equivalence.txt section 5); here that load stays in flight under the first rows.
__global__ __launch_bounds__(kBlock) void k_pool_cat_coalitions_rows(const float* __restrict__ x_atoms, const float* __restrict__ x_frags,
                                                                     fn_seg_plan sa, fn_seg_plan sf, const int8_t* __restrict__ atom_bit,
                                                                     const int32_t* __restrict__ row_mol, const uint64_t* __restrict__ row_mask,
                                                                     float* __restrict__ out) {
    __shared__ float sS[kRows][FN_D];
    const fn_seg_plan& sp = blockIdx.y ? sf : sa;
    const float* src = blockIdx.y ? x_frags : x_atoms;
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int64_t r = blockIdx.x;
    const int64_t s = row_mol[r];
    const uint64_t mask = row_mask[r];
    const int beg = sp.rowptr[s] - sp.pos_base, deg = sp.rowptr[s + 1] - sp.rowptr[s];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = hw; i < deg; i += kRows) {
        const int32_t row = sp.perm[beg + i];
        const int b = blockIdx.y ? -1 : (int)atom_bit[row];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (b < 0 || ((mask >> (unsigned)b) & 1ull)) v = ld4(src + (size_t)row * FN_D + lane * 4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    st4(&sS[hw][lane * 4], acc);
    __syncthreads();
    if (threadIdx.x < FN_D) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kRows; ++w) v += sS[w][threadIdx.x];
        out[(size_t)r * 2 * FN_D + blockIdx.y * FN_D + threadIdx.x] = v;
    }
}

// One whole output row by ONE half-wave: the eight partial rows of block_rows_sum (partial w = items w, w + 8, ... in ascending order)
// live in registers and are added as ((0 + p0) + p1) + ... + p7: another body, the order it reproduces is block_rows_sum's.
// kStaged: item i is row i of `src` (LDS) and `bit` is indexed by i; else item i is row perm[i] of `src` (global memory) and `bit` by
// that row.  bit == nullptr: nothing is masked.
template <bool kStaged>
__device__ __forceinline__ float4 coalition_row(const float* src, const int32_t* __restrict__ perm, const int8_t* bit, int deg,
                                                uint64_t mask, int lane) {
    float4 p[kRows];
#pragma unroll
    for (int w = 0; w < kRows; ++w) p[w] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i0 = 0; i0 < deg; i0 += kRows) {
#pragma unroll
        for (int w = 0; w < kRows; ++w) {
            const int i = i0 + w;
            if (i < deg) {
                const int32_t row = kStaged ? i : perm[i];
                const int b = bit ? (int)bit[row] : -1;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (b < 0 || ((mask >> (unsigned)b) & 1ull)) v = ld4(src + (size_t)row * FN_D + lane * 4);
                p[w].x += v.x; p[w].y += v.y; p[w].z += v.z; p[w].w += v.w;
            }
        }
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int w = 0; w < kRows; ++w) { acc.x += p[w].x; acc.y += p[w].y; acc.z += p[w].z; acc.w += p[w].w; }
    return acc;
}

// The tiled form: a workgroup owns the tile of kCoTile consecutive output rows blockIdx.x and walks the runs of equal row_mol in it
// (row_mol is non-decreasing, so a molecule's rows are one run; a run that crosses a tile boundary belongs to both tiles).  Half-wave hw
// takes the tile's rows hw, hw + 8, ... that lie in the run, each whole (coalition_row), and writes both halves: no cross-wave traffic.
// A run of at least min_run rows whose molecule has at most kCoStage atoms is STAGED: the molecule's atom rows and atom_bit values go
// to LDS once, in pooling order, half-wave 0 adds the fragment rows into sF, one barrier before the rows and one behind them.  A 512-B
// LDS row per atom and a 16-byte read per lane: the 16-lane groups of ds_read_b128 inside a half-wave cover 64 distinct banks, the two
// half-waves of a wave are separate groups -- no conflict, no padding.  Any other run takes the same loop over global memory, without
// LDS and without barriers: a short run would pay the staging round trip for nothing (2048 rows at 4 per molecule: 93 us with every run
// staged against 7 us one workgroup per row).
constexpr int kCoTile = 64, kCoStage = 112, kCoMinRun = 16, kCoAutoRows = 64;
__global__ __launch_bounds__(kBlock) void k_pool_cat_coalitions(const float* __restrict__ x_atoms, const float* __restrict__ x_frags,
                                                                fn_seg_plan sa, fn_seg_plan sf, const int8_t* __restrict__ atom_bit,
                                                                const int32_t* __restrict__ row_mol, const uint64_t* __restrict__ row_mask,
                                                                int64_t R, int min_run, float* __restrict__ out) {
    __shared__ float sX[kCoStage * FN_D];
    __shared__ float sF[FN_D];
    __shared__ int32_t sMol[kCoTile];
    __shared__ unsigned long long sStarts;
    __shared__ int8_t sBit[kCoStage];
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * kCoTile;
    const int n = (int)((R - r0) < (int64_t)kCoTile ? (R - r0) : (int64_t)kCoTile);
    if (threadIdx.x < kCoTile) {                     // wave 0: the tile's molecules and the first row of every run
        const int t = threadIdx.x;
        const int32_t m = t < n ? row_mol[r0 + t] : -1;
        const int32_t before = (t > 0 && t < n) ? row_mol[r0 + t - 1] : -1;
        sMol[t] = m;
        const unsigned long long first = __ballot(t < n && (t == 0 || m != before));
        if (t == 0) sStarts = first;
    }
    __syncthreads();
    unsigned long long starts = sStarts;
    while (starts) {                                 // uniform over the workgroup, and so is `staged`
        const int a = __ffsll(starts) - 1;
        starts &= starts - 1;
        const int e = starts ? __ffsll(starts) - 1 : n;
        const int64_t s = sMol[a];
        const int beg = sa.rowptr[s] - sa.pos_base, deg = sa.rowptr[s + 1] - sa.rowptr[s];
        const int fbeg = sf.rowptr[s] - sf.pos_base, fdeg = sf.rowptr[s + 1] - sf.rowptr[s];
        const bool staged = deg <= kCoStage && e - a >= min_run;
        if (staged) {
            if (hw == 0) st4(&sF[lane * 4], coalition_row<false>(x_frags, sf.perm + fbeg, nullptr, fdeg, 0, lane));
            for (int idx = threadIdx.x; idx < deg * 32; idx += kBlock) {
                const int i = idx >> 5, c = idx & 31;
                const int32_t row = sa.perm[beg + i];
                st4(&sX[i * FN_D + c * 4], ld4(x_atoms + (size_t)row * FN_D + c * 4));
                if (c == 0) sBit[i] = atom_bit[row];
            }
            __syncthreads();
        }
        for (int j = a + ((hw - a) & (kRows - 1)); j < e; j += kRows) {
            const uint64_t mask = row_mask[r0 + j];
            float4 acc, frag;
            if (staged) {
                acc = coalition_row<true>(sX, nullptr, sBit, deg, mask, lane);
                frag = ld4(&sF[lane * 4]);
            } else {
                acc = coalition_row<false>(x_atoms, sa.perm + beg, atom_bit, deg, mask, lane);
                frag = coalition_row<false>(x_frags, sf.perm + fbeg, nullptr, fdeg, 0, lane);
            }
            float* o = out + (size_t)(r0 + j) * 2 * FN_D + lane * 4;
            st4(o, acc);
            st4(o + FN_D, frag);
        }
        if (staged) __syncthreads();                 // the next staged run overwrites the staging area
    }
}
// its backward: g_atoms[i,:] = g[batch[i], 0:128], g_frags[f,:] = g[frag_batch[f], 128:256]
__global__ void k_pool_cat_bwd(const float* __restrict__ g, const int64_t* __restrict__ batch, const int64_t* __restrict__ frag_batch,
                               float* __restrict__ g_atoms, float* __restrict__ g_frags, int64_t N, int64_t F) {
    const int64_t total = (N + F) * 32;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i >> 5;
        const int c4 = (int)(i & 31);
        if (r < N) st4(g_atoms + r * FN_D + c4 * 4, ld4(g + batch[r] * 2 * FN_D + c4 * 4));
        else st4(g_frags + (r - N) * FN_D + c4 * 4, ld4(g + frag_batch[r - N] * 2 * FN_D + FN_D + c4 * 4));
    }
}

// loss = sum_i w[i] * sum_t (out[i,t] - y[i,t])^2 / (sum_i w[i] * T) and its gradient w.r.t. out, one block
// (MSELoss of train/utils.py:341 restricted to the rows with weight 1; B*T is a few hundred to a few thousand)
__global__ __launch_bounds__(1024) void k_masked_mse(const float* __restrict__ out, const float* __restrict__ y,
                                                     const float* __restrict__ w, int64_t B, int T, float* __restrict__ loss,
                                                     float* __restrict__ g_out) {
    __shared__ float s16[16];
    __shared__ float sW;
    float sq = 0.f, ws = 0.f;
    for (int64_t i = threadIdx.x; i < B * T; i += 1024) {
        const float d = out[i] - y[i], wi = w[i / T];
        sq = fmaf(wi * d, d, sq);
    }
    for (int64_t i = threadIdx.x; i < B; i += 1024) ws += w[i];
    const float S = block_sum_1024(sq, s16);
    __syncthreads();
    const float W = block_sum_1024(ws, s16);
    const float denom = W * (float)T;
    if (threadIdx.x == 0) { loss[0] = S / denom;  sW = denom; }
    __syncthreads();
    const float scale = 2.f / sW;
    for (int64_t i = threadIdx.x; i < B * T; i += 1024) g_out[i] = scale * w[i / T] * (out[i] - y[i]);
}

// multi-task classification loss (compute_bce_loss, train/utils.py:297-304): BCE-with-logits averaged over the valid
// entries (target > -0.5 = label present, row weight > 0 = real molecule) and its gradient, one block
__global__ __launch_bounds__(1024) void k_masked_bce(const float* __restrict__ out, const float* __restrict__ y,
                                                     const float* __restrict__ w, int64_t B, int T, float* __restrict__ loss,
                                                     float* __restrict__ g_out) {
    __shared__ float s16[16];
    __shared__ float sN;
    float sum = 0.f, cnt = 0.f;
    for (int64_t i = threadIdx.x; i < B * T; i += 1024) {
        const float x = out[i], t = y[i];
        if (t > -0.5f && w[i / T] > 0.f) {
            const float tt = fmaxf(t, 0.f);
            sum += fmaxf(x, 0.f) - x * tt + log1pf(expf(-fabsf(x)));
            cnt += 1.f;
        }
    }
    const float S = block_sum_1024(sum, s16);
    __syncthreads();
    const float N = block_sum_1024(cnt, s16);
    if (threadIdx.x == 0) { loss[0] = S / N;  sN = N; }
    __syncthreads();
    const float inv = 1.f / sN;
    for (int64_t i = threadIdx.x; i < B * T; i += 1024) {
        const float x = out[i], t = y[i];
        const bool valid = t > -0.5f && w[i / T] > 0.f;
        g_out[i] = valid ? (1.f / (1.f + expf(-x)) - fmaxf(t, 0.f)) * inv : 0.f;
    }
}

// ---- sum_k coef_k * masked_mse_k over up to four (prediction, target, row weight) triples in two multi-block launches:
// pass 1 writes per-block partial (sum w d^2, sum w) of every task, pass 2 lets every block re-add the partials in a
// fixed order (so all blocks agree bit for bit), block 0 writes the total loss and all blocks write their slice of the
// gradients coef_k * 2 / (W_k T_k) * w * (out - y).  coef_k = c_k * (scale_dev[idx_k] if idx_k >= 0 else 1).
constexpr int kMseBlocks = 64;
struct MseTask {
    const float *out, *y, *w;
    float* g;
    int64_t B;
    int T, scale_idx;
    float c;
};
struct MseTasks {
    MseTask t[4];
    int n;
    const float* scale_dev;
};
__global__ __launch_bounds__(256) void k_mse_multi_partial(MseTasks M, float* __restrict__ part /*[n][kMseBlocks][2]*/) {
    __shared__ float s4[4];
    const MseTask& t = M.t[blockIdx.y];
    float sq = 0.f, ws = 0.f;
    const int64_t total = t.B * t.T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)kMseBlocks * 256) {
        const float d = t.out[i] - t.y[i], wi = t.w[i / t.T];
        sq = fmaf(wi * d, d, sq);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < t.B; i += (int64_t)kMseBlocks * 256) ws += t.w[i];
    for (int pass = 0; pass < 2; ++pass) {
        float v = pass ? ws : sq;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) part[((size_t)blockIdx.y * kMseBlocks + blockIdx.x) * 2 + pass] = s4[0] + s4[1] + s4[2] + s4[3];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_mse_multi_finish(MseTasks M, const float* __restrict__ part, float* __restrict__ loss) {
    __shared__ float sS[4], sW[4];
    if (threadIdx.x < M.n) {
        float S = 0.f, W = 0.f;
        for (int b = 0; b < kMseBlocks; ++b) {
            S += part[((size_t)threadIdx.x * kMseBlocks + b) * 2];
            W += part[((size_t)threadIdx.x * kMseBlocks + b) * 2 + 1];
        }
        sS[threadIdx.x] = S;
        sW[threadIdx.x] = W * (float)M.t[threadIdx.x].T;
    }
    __syncthreads();
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        float L = 0.f;
        for (int k = 0; k < M.n; ++k) {
            const float coef = M.t[k].c * (M.t[k].scale_idx >= 0 ? M.scale_dev[M.t[k].scale_idx] : 1.f);
            L += coef * (sS[k] / sW[k]);
        }
        loss[0] = L;
    }
    const MseTask& t = M.t[blockIdx.y];
    const float coef = t.c * (t.scale_idx >= 0 ? M.scale_dev[t.scale_idx] : 1.f);
    const float scale = coef * 2.f / sW[blockIdx.y];
    const int64_t total = t.B * t.T;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)kMseBlocks * 256)
        t.g[i] = scale * t.w[i / t.T] * (t.out[i] - t.y[i]);
}

__global__ void k_segment_sum_any(const float* __restrict__ src, int64_t src_ld, const int32_t* __restrict__ rowptr,
                                  const int32_t* __restrict__ perm, int32_t pos_base, float* __restrict__ out,
                                  int64_t n_seg, int64_t width) {
    const int64_t total = n_seg * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / width, c = i % width;
        const int beg = rowptr[s] - pos_base, deg = rowptr[s + 1] - rowptr[s];
        float acc = 0.f;
        for (int k = 0; k < deg; ++k) acc += src[(size_t)perm[beg + k] * src_ld + c];
        out[i] = acc;
    }
}

// out[i,:] = table[index[i],:] (+ addend[i,:] when given; addend may alias out)
__global__ void k_gather_rows4(const float* __restrict__ table, const int64_t* __restrict__ index,
                               float* out, int64_t rows, int64_t w4, const float* addend) {
    const int64_t total = rows * w4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / w4, c = i % w4;
        float4 v = ld4(table + ((size_t)index[r] * w4 + c) * 4);
        if (addend) { const float4 a = ld4(addend + i * 4); v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w; }
        st4(out + i * 4, v);
    }
}

__global__ void k_gather_rows1(const float* __restrict__ table, const int64_t* __restrict__ index,
                               float* __restrict__ out, int64_t rows, int64_t width) {
    const int64_t total = rows * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = table[(size_t)index[i / width] * width + (i % width)];
}

__global__ void k_segment_softmax(const float* __restrict__ logits, const int32_t* __restrict__ rowptr,
                                  const int32_t* __restrict__ perm, int32_t pos_base, float* __restrict__ probs,
                                  int64_t n_seg, int64_t width) {
    const int64_t total = n_seg * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / width, c = i % width;
        const int beg = rowptr[s] - pos_base, deg = rowptr[s + 1] - rowptr[s];
        float mx = -INFINITY;
        for (int k = 0; k < deg; ++k) mx = fmaxf(mx, logits[(size_t)perm[beg + k] * width + c]);
        float den = 0.f;
        for (int k = 0; k < deg; ++k) den += expf(logits[(size_t)perm[beg + k] * width + c] - mx);
        for (int k = 0; k < deg; ++k) {
            const size_t o = (size_t)perm[beg + k] * width + c;
            probs[o] = expf(logits[o] - mx) / den;
        }
    }
}

__global__ void k_segment_softmax_bwd(const float* __restrict__ probs, const float* __restrict__ g_probs,
                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm,
                                      int32_t pos_base, float* __restrict__ g_logits, int64_t n_seg, int64_t width) {
    const int64_t total = n_seg * width;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / width, c = i % width;
        const int beg = rowptr[s] - pos_base, deg = rowptr[s + 1] - rowptr[s];
        float dot = 0.f;
        for (int k = 0; k < deg; ++k) {
            const size_t o = (size_t)perm[beg + k] * width + c;
            dot = fmaf(probs[o], g_probs[o], dot);
        }
        for (int k = 0; k < deg; ++k) {
            const size_t o = (size_t)perm[beg + k] * width + c;
            g_logits[o] = probs[o] * (g_probs[o] - dot);
        }
    }
}

// =====================================================================================
// dropout + ReLU epilogue (Philox-4x32, seven rounds: philox4x32 in fn_internal.h) and Adam: bodies in shared_bodies.inc
// =====================================================================================
template <bool BWD>
__global__ void k_dropout_act(const float* __restrict__ a, const float* __restrict__ y_saved, float* __restrict__ o,
                              int64_t numel, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                              int relu) {
    dropout_act_body<BWD>(a, y_saved, o, numel, p, seed, offset, offset_dev, relu, (int)blockIdx.x, (int)gridDim.x);
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       int64_t n, float lr_over_bc1, float beta1, float beta2, float eps, float inv_sqrt_bc2, float wd,
                       const int64_t* __restrict__ step_dev, const float* __restrict__ lr_dev) {
    adam_body(p, g, m, v, n, lr_over_bc1, beta1, beta2, eps, inv_sqrt_bc2, wd, step_dev, lr_dev, (int)blockIdx.x, (int)gridDim.x);
}

__global__ void k_edge_concat(const float* __restrict__ x, const float* __restrict__ e_attr,
                              const int64_t* __restrict__ edge_index, float* __restrict__ out, int64_t E) {
    const int64_t total = E * 96;     // float4 slots per row: 3 x 32
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = i / 96;
        const int q = (int)(i % 96);
        float4 v;
        if (q < 32) v = ld4(x + (size_t)edge_index[e] * FN_D + q * 4);
        else if (q < 64) v = ld4(x + (size_t)edge_index[E + e] * FN_D + (q - 32) * 4);
        else v = ld4(e_attr + (size_t)e * FN_D + (q - 64) * 4);
        st4(out + i * 4, v);
    }
}

#include "linear128.inc"

template <int KQ, bool VEC, bool PF>
__global__ __launch_bounds__(kLinThreads) void k_linear128(const float* __restrict__ X, int K, const float* __restrict__ Bt,
                                                   const float* __restrict__ bias, float* __restrict__ Y, int64_t M,
                                                   fn_act_epilogue mk, NodeScalarEpi ns) {
    extern __shared__ __attribute__((aligned(16))) float sBt[];
    linear128_body<KQ, VEC, PF, false, false, false>(sBt, X, K, Bt, bias, Y, M, mk, ns, (int)blockIdx.x, (int)gridDim.x);
}

template <int KQ, bool VEC, bool PF>
__global__ __launch_bounds__(kLinThreads) void k_linear128_multi(LinTasks T) {
    extern __shared__ __attribute__((aligned(16))) float sBt[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const LinTask& t = T.t[ti];
    linear128_body<KQ, VEC, PF>(sBt, t.X, t.K ? t.K : T.K, t.Bt, t.bias, t.Y, t.M, t.mk, t.ns, (int)blockIdx.x - t.first, t.nblk,
                                RowAdd{nullptr, nullptr, 0}, CuEpi{nullptr, nullptr, nullptr, nullptr, nullptr, 0}, t.n_real);
}

// the grouped launch when a task carries a RowAdd term and cannot ride in an attention launch
__global__ __launch_bounds__(kLinThreads) void k_linear128_multi_ra(LinTasks T) {
    extern __shared__ __attribute__((aligned(16))) float sBt[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const LinTask& t = T.t[ti];
    linear128_body<32, true, false, true>(sBt, t.X, 128, t.Bt, t.bias, t.Y, t.M, t.mk, t.ns, (int)blockIdx.x - t.first, t.nblk, t.ra,
                                          CuEpi{nullptr, nullptr, nullptr, nullptr, nullptr, 0}, t.n_real);
}

// layer 0: all three projections read raw features only (K = 17 bond, 6 connection, 167 atom features at the reference's sizes), so
// they share a launch although their reduction lengths need two instantiations of the body: tasks with K <= 20 run the short one,
// the others the K <= 168 one (whose operand tile sets the launch's LDS size)
__global__ __launch_bounds__(kLinThreads) void k_linear128_layer0(LinTasks T) {
    extern __shared__ __attribute__((aligned(16))) float sBt[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const LinTask& t = T.t[ti];
    const RowAdd no_ra{nullptr, nullptr, 0};
    const CuEpi no_cu{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (t.K > 20) linear128_body<44, false, false>(sBt, t.X, t.K, t.Bt, t.bias, t.Y, t.M, t.mk, t.ns, (int)blockIdx.x - t.first, t.nblk, no_ra, no_cu, t.n_real);
    else linear128_body<5, false, false>(sBt, t.X, t.K, t.Bt, t.bias, t.Y, t.M, t.mk, t.ns, (int)blockIdx.x - t.first, t.nblk, no_ra, no_cu, t.n_real);
}

// Bt[k][n] = W[n][k]  (W is nn.Linear.weight [128, K])
__global__ void k_transpose_w(const float* __restrict__ W, int K, float* __restrict__ Bt) {
    __shared__ float tile[32][33];
    const int k0 = blockIdx.x * 32, n0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 thr = 32x8
    for (int r = ty; r < 32; r += 8) tile[r][tx] = (k0 + tx < K) ? W[(size_t)(n0 + r) * K + k0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (k0 + r < K) Bt[(size_t)(k0 + r) * 128 + n0 + tx] = tile[tx][r];
}


// m: the level's edge count (a level without edges has an empty attribute table, whose pointer may be null: nothing reads it)
bool bad_edge_term(const fn_edge_term* et, int64_t m = 1) {      // (the other translation units: fni::bad_edge_term)
    if (!et) return true;
    if (et->mode == 0) return false;
    if (et->mode != 2) return true;
    return et->K < 1 || et->K > FN_MAX_EDGE_K || et->d_e < 1 || et->d_e > 128 || (!et->x_sorted && m > 0) || !et->embW || !et->embb;
}

}  // namespace

// =====================================================================================
// C-ABI
// =====================================================================================
namespace {
unsigned long long* g_mol_stamps = nullptr;     // fn_debug_set_stamps
int64_t g_mol_stamps_n = 0;
hipEvent_t g_prof_ev[4] = {nullptr, nullptr, nullptr, nullptr};      // fn_debug_set_profile_events: forward begin / end, backward begin / end
// records profiling event `i` (if set) on the stream: as an EXTERNAL event node while the stream is being captured, so that the
// time between two of them can be read after a replay of the graph
int prof_event(int i, hipStream_t st) {
    if (!g_prof_ev[i]) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError();  cs = hipStreamCaptureStatusNone; }
    hipError_t rc;
    if (cs != hipStreamCaptureStatusActive) rc = hipEventRecord(g_prof_ev[i], st);
    else {
        rc = hipEventRecordWithFlags(g_prof_ev[i], st, hipEventRecordExternal);
        if (rc != hipSuccess) {      // the same node by hand: an event-record node behind the stream's current capture dependencies
            (void)hipGetLastError();
            hipGraph_t graph = nullptr;
            const hipGraphNode_t* deps = nullptr;
            size_t n_deps = 0;
            unsigned long long id = 0;
            rc = hipStreamGetCaptureInfo_v2(st, &cs, &id, &graph, &deps, &n_deps);
            hipGraphNode_t node = nullptr;
            if (rc == hipSuccess) rc = hipGraphAddEventRecordNode(&node, graph, deps, n_deps, g_prof_ev[i]);
            if (rc == hipSuccess) rc = hipStreamUpdateCaptureDependencies(st, &node, 1, hipStreamSetCaptureDependencies);
        }
    }
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        static thread_local char msg[160];
        snprintf(msg, sizeof msg, "fn_debug_set_profile_events: recording the event failed (%s)", hipGetErrorString(rc));
        return fail(FN_EUNSUPPORTED, msg);
    }
    return 0;
}
int g_tune[FN_TUNE_COUNT] = {1024, 0, 0, 192, 0, 0, 0, 1, 1, 0, 1792, 1536, 512, 512, 2, -1, 0, 1, 0, 0, 1, 23, 1, 768, 1, 0, 1, 1, 0, 0, 6144, 1, 1, 1, 1};   // in the order of the FN_TUNE_* keys
// What fn_set_tuning accepts, in the order of the FN_TUNE_* keys (the ranges stated at the defines in the header).  A block-count key
// is at least 1 and at most what the partial-sum buffers behind its launch hold (every block writes one row of them); the clamps at the
// use sites stay, as the second line of defence of whoever calls a launcher with a table this function did not fill.
struct TuneRange { const char* name; int lo, hi; };
constexpr int kTuneAny = 0x7fffffff, kTuneBlocks = 1 << 20;
constexpr TuneRange kRetired{"retired", -kTuneAny - 1, kTuneAny};
constexpr TuneRange kTuneRange[FN_TUNE_COUNT] = {
    {"FWD_BLOCKS", 1, kTuneBlocks},              //  0
    {"GEMM_SLOTS", 0, kTuneBlocks},              //  1
    kRetired,                                    //  2
    {"WGRAD_BLOCKS", 1, kTuneBlocks},            //  3
    kRetired, kRetired, kRetired,                //  4, 5, 6
    {"FUSE_ROWDOTS", 0, 1},                      //  7
    {"WGRAD_DIRECT", 0, 1},                      //  8
    kRetired,                                    //  9
    {"FWD_BLOCKS_EVAL", 1, kTuneBlocks},         // 10
    {"DST_BLOCKS", 1, FN_MAX_PART},              // 11: a row of part_e per block
    {"SRC_BLOCKS", 1, 1024},                     // 12: prep_gat_bwd_src's bound
    {"RD_BLOCKS", 1, FN_MAX_PART},               // 13: the rows a part_rd table holds
    {"GEMM_COLAUNCH", 0, 2},                     // 14
    kRetired, kRetired, kRetired, kRetired, kRetired,      // 15 .. 19
    {"MOL_TAIL", 0, 2},                          // 20
    {"WGRAD0_ROWS", 1, 99},                      // 21: two decimal digits
    {"BWD_ONE", 0, 1},                           // 22
    {"ONE_BLOCKS", 1, FN_MAX_PART},              // 23: prep_gat_bwd_one's bound
    {"PAD_SKIP", 0, 1},                          // 24
    {"ONE_INTERLEAVE", 0, 1},                    // 25
    {"ONE_TIER6", 0, 1},                         // 26
    {"RIDER_PIECES", 1, 4096},                   // 27
    {"RIDER_AT", 0, 1},                          // 28
    kRetired,                                    // 29
    {"FWD_BLOCKS_EVAL_LARGE", 0, kTuneBlocks},   // 30
    {"FWD_TAIL_ROWS", 0, kTuneBlocks},           // 31
    {"DENSE_TILES", 0, 1},                       // 32
    {"ENGINE_CONST", 0, 1},                      // 33
    {"COALITION_STAGED", 0, kTuneAny},           // 34
};
}  // namespace
namespace fni {      // hooks for the other translation units (fn_internal.h)
int fail(int code, const char* what) { return ::fail(code, what); }
int launch_status(const char* where) { return ::launch_status(where); }
int tune(int key) { return key >= 0 && key < FN_TUNE_COUNT ? g_tune[key] : 0; }
unsigned long long* stamps(int64_t* n_u64) { *n_u64 = g_mol_stamps_n;  return g_mol_stamps; }
bool bad_edge_term(const fn_edge_term* et, int64_t m) { return ::bad_edge_term(et, m); }
}  // namespace fni
namespace {
// blocks of a product with `tiles` row tiles when every block walks `iters` of them (two column halves per tile)
inline int lin_iters(int64_t total_tiles) {     // row tiles per block so that the launch is resident at once (four blocks per CU)
    const int64_t slots = g_tune[FN_TUNE_GEMM_SLOTS];
    if (slots <= 0) return 1;                   // default: one output tile per workgroup (measured best, tools/probe/gemm_probe.hip)
    const int64_t it = (2 * total_tiles + slots - 1) / slots;
    return (int)(it < 1 ? 1 : it);
}
template <int KQ>
int launch_linear128(const float* X, int K, const float* Bt, const float* bias, float* Y, int64_t M, fn_act_epilogue mk,
                     NodeScalarEpi ns, hipStream_t st) {
    const size_t lds = (size_t)(4 * KQ * kLinLd) * sizeof(float);
    const int64_t tiles = (M + kLinRows - 1) / kLinRows;
    const int iters = lin_iters(tiles), grid = lin_blocks(tiles, iters);
    constexpr bool VEC = KQ % 4 == 0;
    if (VEC && K == 4 * KQ) {
        if (iters > 1) {
            if (int rc = allow_lds(k_linear128<KQ, VEC, VEC>, lds)) return rc;
            hipLaunchKernelGGL((k_linear128<KQ, VEC, VEC>), dim3(grid), dim3(kLinThreads), lds, st, X, K, Bt, bias, Y, M, mk, ns);
        } else {
            if (int rc = allow_lds(k_linear128<KQ, VEC, false>, lds)) return rc;
            hipLaunchKernelGGL((k_linear128<KQ, VEC, false>), dim3(grid), dim3(kLinThreads), lds, st, X, K, Bt, bias, Y, M, mk, ns);
        }
    } else {
        if (int rc = allow_lds(k_linear128<KQ, false, false>, lds)) return rc;
        hipLaunchKernelGGL((k_linear128<KQ, false, false>), dim3(grid), dim3(kLinThreads), lds, st, X, K, Bt, bias, Y, M, mk, ns);
    }
    return 0;
}
int linear128_group_impl(LinTasks& T, hipStream_t st) {
    constexpr int KQ = 32;
    const size_t lds = (size_t)(4 * KQ * kLinLd) * sizeof(float);
    int64_t total = 0;
    for (int i = 0; i < T.n; ++i) total += T.t[i].M > 0 ? (T.t[i].M + kLinRows - 1) / kLinRows : 0;
    const int iters = lin_iters(total);
    int blocks = lin_layout(T, kLinRows, iters);
    T.K = 128;
    if (!T.n) return 0;
    bool any_ra = false;
    for (int i = 0; i < T.n; ++i) any_ra |= T.t[i].ra.z != nullptr;
    if (any_ra) {                          // a RowAdd term must not get lost: the kernel variant that applies it (one tile per workgroup)
        blocks = lin_layout(T, kLinRows, 1);
        hipLaunchKernelGGL(k_linear128_multi_ra, dim3(blocks), dim3(kLinThreads), lds, st, T);
        return launch_status("grouped projection GEMM (+ row term)");
    }
    if (iters > 1) {
        if (int rc = allow_lds(k_linear128_multi<KQ, true, true>, lds)) return rc;
        hipLaunchKernelGGL((k_linear128_multi<KQ, true, true>), dim3(blocks), dim3(kLinThreads), lds, st, T);
    } else {
        if (int rc = allow_lds(k_linear128_multi<KQ, true, false>, lds)) return rc;
        hipLaunchKernelGGL((k_linear128_multi<KQ, true, false>), dim3(blocks), dim3(kLinThreads), lds, st, T);
    }
    return launch_status("grouped projection GEMM");
}

// layer 0: the bond (K = 17) and connection (K = 6) projections in one launch of the K <= 20 variant, each task with its own K
int launch_linear128_small_group(LinTasks& T, hipStream_t st) {
    constexpr int KQ = 5;
    bool mixed = false;                          // a task with 20 < K <= 168 rides along (k_linear128_layer0)
    for (int i = 0; i < T.n; ++i) mixed |= T.t[i].M > 0 && T.t[i].K > 4 * KQ;
    const size_t lds = (size_t)(4 * (mixed ? 44 : KQ) * kLinLd) * sizeof(float);
    for (int i = 0; i < T.n; ++i)
        if (T.t[i].M > 0 && (T.t[i].K < 1 || T.t[i].K > 168)) return fail(FN_EINVAL, "layer-0 projection group: K must be 1..168");
    const int blocks = lin_layout(T, kLinRows, 1);
    T.K = 4 * KQ;
    if (!T.n) return 0;
    if (mixed) hipLaunchKernelGGL(k_linear128_layer0, dim3(blocks), dim3(kLinThreads), lds, st, T);
    else hipLaunchKernelGGL((k_linear128_multi<KQ, false, false>), dim3(blocks), dim3(kLinThreads), lds, st, T);
    return launch_status("grouped projection GEMM (layer 0)");
}

// fn_linear128_f32, with the node scalars of the level the rows feed as an optional epilogue (the engine: fni::launch_linear128_ns)
int linear128_impl(const float* X, int K, const float* Bt, const float* bias, float* Y, int64_t M, const fn_act_epilogue* act_bwd,
                   NodeScalarEpi ns, fn_stream_t stream) {
    if (K < 1 || M < 0) return fail(FN_EINVAL, "fn_linear128_f32: bad argument");
    const fn_act_epilogue mk = act_bwd ? *act_bwd : fn_act_epilogue{nullptr, 0.f, 0, 0, 0, nullptr};
    if (M == 0) return 0;
    if (!X || !Bt || !Y || (((uintptr_t)X | (uintptr_t)Y) & 15)) return fail(FN_EINVAL, "fn_linear128_f32: null or misaligned buffer");
    int rc;
    if (K <= 8) rc = launch_linear128<2>(X, K, Bt, bias, Y, M, mk, ns, S(stream));
    else if (K <= 20) rc = launch_linear128<5>(X, K, Bt, bias, Y, M, mk, ns, S(stream));
    else if (K <= 128) rc = launch_linear128<32>(X, K, Bt, bias, Y, M, mk, ns, S(stream));
    else if (K <= 168) rc = launch_linear128<44>(X, K, Bt, bias, Y, M, mk, ns, S(stream));
    else return fail(FN_EUNSUPPORTED, "fn_linear128_f32: K > 168");
    if (rc) return rc;
    return launch_status("fn_linear128_f32");
}
}  // namespace

namespace fni {      // launchers of this unit's kernels that the engine (encoder.hip) calls
int prof_event(int i, hipStream_t st) { return ::prof_event(i, st); }
int launch_linear128_group(LinTasks& T, hipStream_t st) { return ::linear128_group_impl(T, st); }
int launch_linear128_small_group(LinTasks& T, hipStream_t st) { return ::launch_linear128_small_group(T, st); }
int launch_linear128_ns(const float* X, int K, const float* Bt, const float* bias, float* Y, int64_t M, const fn_act_epilogue* act_bwd, NodeScalarEpi ns,
                        fn_stream_t stream) {
    return ::linear128_impl(X, K, Bt, bias, Y, M, act_bwd, ns, stream);
}
int launch_gather_rows4(const float* table, const int64_t* index, float* out, int64_t rows, int64_t w4, const float* addend, hipStream_t st,
                        const char* where) {
    hipLaunchKernelGGL(k_gather_rows4, dim3(flat_grid(rows * w4, kGridCap)), dim3(kBlock), 0, st, table, index, out, rows, w4, addend);
    return ::launch_status(where);
}
}  // namespace fni

extern "C" {

int fn_abi_version(void) { return FN_ABI_VERSION; }

int fn_debug_set_stamps(void* buf, int64_t n_u64) {
    g_mol_stamps = static_cast<unsigned long long*>(buf);
    g_mol_stamps_n = buf ? n_u64 : 0;
    return 0;
}

int fn_debug_set_profile_events(void* const* events) {
    for (int i = 0; i < 4; ++i) g_prof_ev[i] = events ? static_cast<hipEvent_t>(events[i]) : nullptr;
    return 0;
}

int fn_set_tuning(int key, int value) {
    if (key < 0 || key >= FN_TUNE_COUNT) return fail(FN_EINVAL, "fn_set_tuning: unknown key");
    const TuneRange& r = kTuneRange[key];
    if (value < r.lo || value > r.hi) {
        static thread_local char msg[160];
        snprintf(msg, sizeof msg, "fn_set_tuning: key %d (%s) takes %d .. %d, not %d", key, r.name, r.lo, r.hi, value);
        return fail(FN_EINVAL, msg);
    }
    g_tune[key] = value;
    return 0;
}
int fn_get_tuning(int key) { return fni::tune(key); }
const char* fn_last_error(void) { return tl_err; }



int fn_node_scalars_f32(const float* h, const float* att, int att_w, int dst_off, int src_off, float* s_dst,
                        float* s_src, int64_t n, int heads, fn_stream_t stream) {
    if (!h || !att || !s_dst || !s_src || n < 0) return fail(FN_EINVAL, "fn_node_scalars_f32: bad argument");
    if ((att_w | dst_off | src_off) & 3) return fail(FN_EINVAL, "fn_node_scalars_f32: att blocks must be 16-byte aligned");
    if (n == 0) return 0;
    FN_TRY(with_heads(heads, [&](auto H) {
        hipLaunchKernelGGL(k_node_scalars<FN_CV(H)>, dim3(row_grid(n, kGridCap)), dim3(kBlock), 0, S(stream), h, att, att_w, dst_off, src_off, s_dst, s_src, n);
    }));
    return launch_status("fn_node_scalars_f32");
}

static int launch_gat_bwd_dst(const GatBwdDstArgs& A, int heads, hipStream_t st) {
    if (A.nblk == 0) return 0;
    const int kl = edge_class(&A.et);
    FN_TRY(with_heads(heads, [&](auto H) { with_edge_class(kl, [&](auto KL) {
        hipLaunchKernelGGL((k_gat_bwd_dst<FN_CV(H), FN_CV(KL), kBwdRows>), dim3(A.nblk), dim3(kBwdRows * 32), 0, st, A);
    }); }));
    return launch_status("fn_gat_bwd_dst_f32");
}


int fn_gat_bwd_dst_f32(const float* g_out, const float* h, const float* p_sorted, const fn_edge_term* et,
                       const fn_gat_plan* plan, float neg_slope, float* dz_sorted, float* g_s_orig, float* pz_src,
                       float* g_s_dst, float* part_e, int* n_part_e, int heads, fn_stream_t stream) {
    GatBwdDstArgs A;
    if (int rc = prep_gat_bwd_dst(g_out, h, p_sorted, et, plan, neg_slope, dz_sorted, g_s_orig, pz_src, g_s_dst, part_e, n_part_e, heads, &A)) return rc;
    return launch_gat_bwd_dst(A, heads, S(stream));
}

int fn_attn_by_src_f32(const float* p_sorted, const fn_gat_plan* plan, float* attn, int heads, fn_stream_t stream) {
    if (!plan || !attn || (plan->m > 0 && !p_sorted)) return fail(FN_EINVAL, "fn_attn_by_src_f32: bad argument");
    if (plan->n == 0) return 0;
    FN_TRY(with_heads(heads, [&](auto H) {
        hipLaunchKernelGGL(k_attn_by_src<FN_CV(H)>, dim3(flat_grid(plan->n * heads, kGridCap)), dim3(kBlock), 0, S(stream), p_sorted, *plan, attn);
    }));
    return launch_status("fn_attn_by_src_f32");
}

int fn_row_dots_sorted_f32(const float* feat, const float* A, int lda, int off, int J, const fn_gat_plan* plan,
                           float* s_sorted, fn_stream_t stream) {
    if (!A || !plan || J < 1 || J > 8 || ((lda | off) & 3)) return fail(FN_EINVAL, "fn_row_dots_sorted_f32: bad argument");
    if (plan->m == 0) return 0;
    if (!s_sorted || (plan->m_real > 0 && !feat)) return fail(FN_EINVAL, "fn_row_dots_sorted_f32: null buffer");
    hipLaunchKernelGGL(k_row_dots_sorted, dim3(row_grid(plan->m, kGridCap)), dim3(kBlock), 0, S(stream), feat, A, lda, off, J,
                       *plan, s_sorted);
    return launch_status("fn_row_dots_sorted_f32");
}

int fn_colsum_f32(const float* part, int n_rows, int cols, float* out, int ld, int off, fn_stream_t stream) {
    if (!part || !out || n_rows < 0 || n_rows > FN_MAX_PART || cols < 1) return fail(FN_EINVAL, "fn_colsum_f32: bad argument");
    hipLaunchKernelGGL(k_colsum, dim3(cols), dim3(1024), 0, S(stream), part, n_rows, cols, out, ld, off);
    return launch_status("fn_colsum_f32");
}

int fn_transpose_w_f32(const float* W, int K, float* Bt, fn_stream_t stream) {
    if (!W || !Bt || K < 1) return fail(FN_EINVAL, "fn_transpose_w_f32: bad argument");
    hipLaunchKernelGGL(k_transpose_w, dim3((K + 31) / 32, 4), dim3(256), 0, S(stream), W, K, Bt);
    return launch_status("fn_transpose_w_f32");
}

int fn_linear128_f32(const float* X, int K, const float* Bt, const float* bias, float* Y, int64_t M,
                     const fn_act_epilogue* act_bwd, fn_stream_t stream) {
    return linear128_impl(X, K, Bt, bias, Y, M, act_bwd, NodeScalarEpi{nullptr, nullptr, nullptr, 0, 0, 0, 0}, stream);
}

int fn_segment_sum_f32(const float* src, int64_t src_ld, const int32_t* rowptr, const int32_t* perm, int32_t pos_base,
                       float* out, int64_t n_seg, int64_t width, int64_t n_items, fn_stream_t stream) {
    if (!rowptr || !out || n_seg < 0 || width < 1 || src_ld < width) return fail(FN_EINVAL, "fn_segment_sum_f32: bad argument");
    if (n_seg == 0) return 0;
    if (!src || !perm) return fail(FN_EINVAL, "fn_segment_sum_f32: null src/perm");
    if (width == FN_D && (src_ld & 3) == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0) {
        if (n_items >= 4 * n_seg)
            hipLaunchKernelGGL(k_segment_sum128_wide, dim3((unsigned)(n_seg < 8 * kGridCap ? n_seg : 8 * kGridCap)), dim3(kBlock), 0,
                               S(stream), src, src_ld, rowptr, perm, pos_base, out, n_seg);
        else
            hipLaunchKernelGGL(k_segment_sum128, dim3(row_grid(n_seg, kGridCap)), dim3(kBlock), 0, S(stream), src, src_ld, rowptr,
                               perm, pos_base, out, n_seg);
    }
    else
        hipLaunchKernelGGL(k_segment_sum_any, dim3(flat_grid(n_seg * width, kGridCap)), dim3(kBlock), 0, S(stream), src, src_ld,
                           rowptr, perm, pos_base, out, n_seg, width);
    return launch_status("fn_segment_sum_f32");
}

int fn_gather_rows_f32(const float* table, const int64_t* index, float* out, int64_t rows, int64_t width, fn_stream_t stream) {
    if (rows < 0 || width < 1 || !out) return fail(FN_EINVAL, "fn_gather_rows_f32: bad argument");
    if (rows == 0) return 0;
    if (!table || !index) return fail(FN_EINVAL, "fn_gather_rows_f32: null table/index");
    if ((width & 3) == 0 && (((uintptr_t)table | (uintptr_t)out) & 15) == 0)
        return fni::launch_gather_rows4(table, index, out, rows, width / 4, nullptr, S(stream), "fn_gather_rows_f32");
    else
        hipLaunchKernelGGL(k_gather_rows1, dim3(flat_grid(rows * width, kGridCap)), dim3(kBlock), 0, S(stream), table, index, out,
                           rows, width);
    return launch_status("fn_gather_rows_f32");
}

int fn_segment_softmax_f32(const float* logits, const int32_t* rowptr, const int32_t* perm, int32_t pos_base, float* probs,
                           int64_t n_seg, int64_t width, fn_stream_t stream) {
    if (!rowptr || n_seg < 0 || width < 1) return fail(FN_EINVAL, "fn_segment_softmax_f32: bad argument");
    if (n_seg == 0) return 0;
    if (!logits || !perm || !probs) return fail(FN_EINVAL, "fn_segment_softmax_f32: null buffer");
    hipLaunchKernelGGL(k_segment_softmax, dim3(flat_grid(n_seg * width, kGridCap)), dim3(kBlock), 0, S(stream), logits, rowptr,
                       perm, pos_base, probs, n_seg, width);
    return launch_status("fn_segment_softmax_f32");
}

int fn_segment_softmax_bwd_f32(const float* probs, const float* g_probs, const int32_t* rowptr, const int32_t* perm,
                               int32_t pos_base, float* g_logits, int64_t n_seg, int64_t width, fn_stream_t stream) {
    if (!rowptr || n_seg < 0 || width < 1) return fail(FN_EINVAL, "fn_segment_softmax_bwd_f32: bad argument");
    if (n_seg == 0) return 0;
    if (!probs || !g_probs || !perm || !g_logits) return fail(FN_EINVAL, "fn_segment_softmax_bwd_f32: null buffer");
    hipLaunchKernelGGL(k_segment_softmax_bwd, dim3(flat_grid(n_seg * width, kGridCap)), dim3(kBlock), 0, S(stream), probs,
                       g_probs, rowptr, perm, pos_base, g_logits, n_seg, width);
    return launch_status("fn_segment_softmax_bwd_f32");
}

int fn_dropout_act_f32(const float* x, float* y, int64_t numel, float p, uint64_t seed, uint64_t offset,
                       const uint64_t* offset_dev, int relu, fn_stream_t stream) {
    if (numel < 0 || p < 0.f || p > 1.f) return fail(FN_EINVAL, "fn_dropout_act_f32: bad argument");
    if (numel == 0) return 0;
    if (!x || !y || (((uintptr_t)x | (uintptr_t)y) & 15)) return fail(FN_EINVAL, "fn_dropout_act_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_dropout_act<false>, dim3(flat_grid((numel + 3) / 4, kGridCap)), dim3(kBlock), 0, S(stream), x,
                       (const float*)nullptr, y, numel, p, seed, offset, offset_dev, relu);
    return launch_status("fn_dropout_act_f32");
}

int fn_dropout_act_bwd_f32(const float* g_y, const float* y, float* g_x, int64_t numel, float p, uint64_t seed,
                           uint64_t offset, const uint64_t* offset_dev, int relu, fn_stream_t stream) {
    if (numel < 0 || p < 0.f || p > 1.f) return fail(FN_EINVAL, "fn_dropout_act_bwd_f32: bad argument");
    if (numel == 0) return 0;
    if (!g_y || !g_x || (relu && !y) || (((uintptr_t)g_y | (uintptr_t)g_x | (uintptr_t)y) & 15))
        return fail(FN_EINVAL, "fn_dropout_act_bwd_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_dropout_act<true>, dim3(flat_grid((numel + 3) / 4, kGridCap)), dim3(kBlock), 0, S(stream), g_y, y, g_x,
                       numel, p, seed, offset, offset_dev, relu);
    return launch_status("fn_dropout_act_bwd_f32");
}


int fn_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int64_t step, fn_stream_t stream) {
    if (n < 0 || step < 1) return fail(FN_EINVAL, "fn_adam_f32: bad argument");
    if (n == 0) return 0;
    if (!p || !g || !m || !v || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15))
        return fail(FN_EINVAL, "fn_adam_f32: null or misaligned buffer");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(k_adam, dim3(flat_grid((n + 3) / 4, kGridCap)), dim3(kBlock), 0, S(stream), p, g, m, v, n,
                       (float)((double)lr / bc1), beta1, beta2, eps, (float)(1.0 / sqrt(bc2)), weight_decay,
                       (const int64_t*)nullptr, (const float*)nullptr);
    return launch_status("fn_adam_f32");
}

int fn_adam_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                    float eps, float weight_decay, const int64_t* step_dev, fn_stream_t stream) {
    if (n < 0 || !lr_dev || !step_dev) return fail(FN_EINVAL, "fn_adam_dev_f32: bad argument");
    if (n == 0) return 0;
    if (!p || !g || !m || !v || (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15))
        return fail(FN_EINVAL, "fn_adam_dev_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_adam, dim3(flat_grid((n + 3) / 4, kGridCap)), dim3(kBlock), 0, S(stream), p, g, m, v, n, 0.f, beta1, beta2,
                       eps, 0.f, weight_decay, step_dev, lr_dev);
    return launch_status("fn_adam_dev_f32");
}

int fn_edge_concat_f32(const float* x, const float* e_attr, const int64_t* edge_index, float* out, int64_t E,
                       fn_stream_t stream) {
    if (E < 0) return fail(FN_EINVAL, "fn_edge_concat_f32: bad argument");
    if (E == 0) return 0;
    if (!x || !e_attr || !edge_index || !out) return fail(FN_EINVAL, "fn_edge_concat_f32: null buffer");
    hipLaunchKernelGGL(k_edge_concat, dim3(flat_grid(E * 96, kGridCap)), dim3(kBlock), 0, S(stream), x, e_attr, edge_index, out, E);
    return launch_status("fn_edge_concat_f32");
}

int fn_pool_cat_f32(const float* x_atoms, const float* x_frags, const fn_seg_plan* mol_atoms, const fn_seg_plan* mol_frags,
                    float* out, fn_stream_t stream) {
    if (!mol_atoms || !mol_frags || !out || mol_atoms->n_seg != mol_frags->n_seg) return fail(FN_EINVAL, "fn_pool_cat_f32: bad argument");
    if (mol_atoms->n_seg == 0) return 0;
    if ((mol_atoms->n_items > 0 && !x_atoms) || (mol_frags->n_items > 0 && !x_frags) || !mol_atoms->rowptr || !mol_frags->rowptr)
        return fail(FN_EINVAL, "fn_pool_cat_f32: null buffer");
    hipLaunchKernelGGL(k_pool_cat, dim3((unsigned)mol_atoms->n_seg, 2), dim3(kBlock), 0, S(stream), x_atoms, x_frags, *mol_atoms,
                       *mol_frags, out);
    return launch_status("fn_pool_cat_f32");
}

namespace {
// what fn_pool_cat_groups_f32 and fn_pool_cat_coalitions_f32 check alike; atom_vec / row_vec: the per-atom and the per-row vector of
// the read-out.  0 with R == 0: nothing to launch
static int readout_args(const char* fn, const float* x_atoms, const float* x_frags, const fn_seg_plan* mol_atoms, const fn_seg_plan* mol_frags,
                        const void* atom_vec, const int32_t* row_mol, const void* row_vec, int64_t R, const float* out) {
    const char* what = nullptr;
    if (!mol_atoms || !mol_frags || mol_atoms->n_seg != mol_frags->n_seg || R < 0 || R > 0x7fffffffLL) what = "bad argument";
    else if (R == 0) return 0;
    else if (mol_atoms->n_seg == 0) what = "output rows of a batch without molecules";
    else if (!out || !row_mol || !row_vec || (mol_atoms->n_items > 0 && (!x_atoms || !atom_vec || !mol_atoms->perm)) ||
             (mol_frags->n_items > 0 && (!x_frags || !mol_frags->perm)) || !mol_atoms->rowptr || !mol_frags->rowptr)
        what = "null buffer";
    if (!what) return 0;
    char text[128];
    snprintf(text, sizeof(text), "%s: %s", fn, what);
    return fail(FN_EINVAL, text);
}
}  // namespace

int fn_pool_cat_groups_f32(const float* x_atoms, const float* x_frags, const fn_seg_plan* mol_atoms, const fn_seg_plan* mol_frags,
                           const int64_t* atom_group, const int32_t* row_mol, const int64_t* row_group, int64_t R, float* out,
                           fn_stream_t stream) {
    const int rc = readout_args("fn_pool_cat_groups_f32", x_atoms, x_frags, mol_atoms, mol_frags, atom_group, row_mol, row_group, R, out);
    if (rc || R == 0) return rc;
    hipLaunchKernelGGL(k_pool_cat_groups, dim3((unsigned)R, 2), dim3(kBlock), 0, S(stream), x_atoms, x_frags, *mol_atoms, *mol_frags,
                       atom_group, row_mol, row_group, out);
    return launch_status("fn_pool_cat_groups_f32");
}

int fn_pool_cat_coalitions_f32(const float* x_atoms, const float* x_frags, const fn_seg_plan* mol_atoms, const fn_seg_plan* mol_frags,
                               const int8_t* atom_bit, const int32_t* row_mol, const uint64_t* row_mask, int64_t R, float* out,
                               fn_stream_t stream) {
    const int rc = readout_args("fn_pool_cat_coalitions_f32", x_atoms, x_frags, mol_atoms, mol_frags, atom_bit, row_mol, row_mask, R, out);
    if (rc || R == 0) return rc;
    const int form = fni::tune(FN_TUNE_COALITION_STAGED);
    // the tiled form measured faster from 64 rows per molecule on (1.03 - 1.06 x there, 1.4 x at 1024); below it, one workgroup per row is
    if (form == 0 || (form == 1 && R < (int64_t)kCoAutoRows * mol_atoms->n_seg))
        hipLaunchKernelGGL(k_pool_cat_coalitions_rows, dim3((unsigned)R, 2), dim3(kBlock), 0, S(stream), x_atoms, x_frags, *mol_atoms,
                           *mol_frags, atom_bit, row_mol, row_mask, out);
    else
        hipLaunchKernelGGL(k_pool_cat_coalitions, dim3((unsigned)((R + kCoTile - 1) / kCoTile)), dim3(kBlock), 0, S(stream), x_atoms, x_frags,
                           *mol_atoms, *mol_frags, atom_bit, row_mol, row_mask, R, form == 1 ? kCoMinRun : form - 1, out);
    return launch_status("fn_pool_cat_coalitions_f32");
}

int fn_pool_cat_bwd_f32(const float* g, const int64_t* batch, const int64_t* frag_batch, float* g_atoms, float* g_frags,
                        int64_t N, int64_t F, fn_stream_t stream) {
    if (N < 0 || F < 0) return fail(FN_EINVAL, "fn_pool_cat_bwd_f32: bad argument");
    if (N + F == 0) return 0;
    if (!g || (N && (!batch || !g_atoms)) || (F && (!frag_batch || !g_frags))) return fail(FN_EINVAL, "fn_pool_cat_bwd_f32: null buffer");
    hipLaunchKernelGGL(k_pool_cat_bwd, dim3(flat_grid((N + F) * 32, kGridCap)), dim3(kBlock), 0, S(stream), g, batch, frag_batch,
                       g_atoms, g_frags, N, F);
    return launch_status("fn_pool_cat_bwd_f32");
}

int fn_masked_mse_f32(const float* out, const float* y, const float* w, int64_t B, int T, float* loss, float* g_out,
                      fn_stream_t stream) {
    if (!out || !y || !w || !loss || !g_out || B < 1 || T < 1) return fail(FN_EINVAL, "fn_masked_mse_f32: bad argument");
    hipLaunchKernelGGL(k_masked_mse, dim3(1), dim3(1024), 0, S(stream), out, y, w, B, T, loss, g_out);
    return launch_status("fn_masked_mse_f32");
}

int fn_masked_bce_f32(const float* out, const float* y, const float* w, int64_t B, int T, float* loss, float* g_out,
                      fn_stream_t stream) {
    if (!out || !y || !w || !loss || !g_out || B < 1 || T < 1) return fail(FN_EINVAL, "fn_masked_bce_f32: bad argument");
    hipLaunchKernelGGL(k_masked_bce, dim3(1), dim3(1024), 0, S(stream), out, y, w, B, T, loss, g_out);
    return launch_status("fn_masked_bce_f32");
}

int64_t fn_masked_mse_multi_ws(int n_tasks) { return n_tasks > 0 ? (int64_t)n_tasks * kMseBlocks * 2 : 0; }

int fn_masked_mse_multi_f32(const fn_mse_task* tasks, int n_tasks, const float* scale_dev, float* ws, float* loss, fn_stream_t stream) {
    if (!tasks || n_tasks < 1 || n_tasks > 4 || !ws || !loss) return fail(FN_EINVAL, "fn_masked_mse_multi_f32: bad argument");
    MseTasks M{};
    M.n = n_tasks;
    M.scale_dev = scale_dev;
    for (int k = 0; k < n_tasks; ++k) {
        const fn_mse_task& t = tasks[k];
        if (!t.out || !t.y || !t.w || !t.g_out || t.B < 1 || t.T < 1 || (t.scale_idx >= 0 && !scale_dev))
            return fail(FN_EINVAL, "fn_masked_mse_multi_f32: bad task");
        M.t[k] = MseTask{t.out, t.y, t.w, t.g_out, t.B, t.T, t.scale_idx, t.coef};
    }
    hipLaunchKernelGGL(k_mse_multi_partial, dim3(kMseBlocks, n_tasks), dim3(256), 0, S(stream), M, ws);
    hipLaunchKernelGGL(k_mse_multi_finish, dim3(kMseBlocks, n_tasks), dim3(256), 0, S(stream), M, ws, loss);
    return launch_status("fn_masked_mse_multi_f32");
}



}  // extern "C"

