// encoder.hip -- the encoder engine: FragNet.forward and its backward as ONE call each (fn_encoder_forward / fn_encoder_backward and
// their workspace / RNG planners), with every kernel that nothing but the engine launches: the forward prologue (k_enc_prologue), the
// molecule-resident fragment tail (mol_tail.inc), k_frag_tail, k_gate_many, the input-gradient products with the edge term's
// backward beside them (k_lin_rd_cu, k_gat_bwd_src_rd).  The parameters' gradients -- weight-gradient products, the attention vectors'
// finalize, every reduction of partials -- are param_grads.hip's; the passes here queue them on its fni::ParamGradQueue (level_params).
// A few operator entry points live here with their kernels, because those kernels run a device body that one of the engine's combined
// launches runs as well: the backward of the full-width edge term (fn_row_dots_sorted_bwd_f32: row_dots_sorted_bwd_body), the source
// pass of the two-pass attention backward (fn_gat_bwd_src_f32: gat_bwd_src_body, also in k_gat_bwd_src_rd) and the edge-attribute
// permutations (fn_sort_edge_attr_f32 / _src_f32: the bodies k_enc_prologue runs).  A body and all the kernels that run
// it stay in ONE unit: the compiler's inter-procedural passes run before it inlines the body, so what it knows about the body's
// arguments depends on the callers it sees in the unit -- with the callers in two units these kernels came out with other registers
// and schedules than before (profiles/engine_unit_equivalence.txt section 1); and a __global__ function that is no template can be
// compiled into one unit only.
// A translation unit of its own: what it takes from the other units is the fni:: interface of fn_internal.h (host launchers of
// gat_fwd.hip, gat_fwd_lin.hip, gat_bwd_one.hip and fragnet_hip.hip, param_grads.hip's queue, the tuning table through fni::tune) and single-operator entry
// points of the C-ABI (fn_gat_bwd_dst_f32, fn_gat_fwd_f32, ..); device bodies it shares with fragnet_hip.hip are in .inc files both
// include (gat_fwd.inc, gat_bwd_two.inc, linear128.inc, shared_bodies.inc).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <mutex>
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;
using fni::tune;
using fni::prof_event;
using fni::GatFwdArgs;
using fni::prep_gat_fwd;
using fni::launch_gat_fwd;
using fni::launch_gat_fwd_pair;
using fni::launch_gat_fwd_lin;
using fni::launch_gat_fwd_pair_lin;
using fni::GatBwdOneArgs;
using fni::CuTask;
using fni::CuTasks;
using fni::prep_gat_bwd_one;
using fni::launch_gat_bwd_one3;
using fni::launch_gat_cu;
using fni::launch_linear128_group;
using fni::launch_linear128_small_group;
using fni::launch_linear128_ns;
using fni::launch_gather_rows4;
using fni::ParamGradQueue;

#include "gat_fwd.inc"
#include "gat_bwd_two.inc"
#include "shared_bodies.inc"

constexpr int kRowDotsBwdBlocks = 512;    // blocks of k_row_dots_sorted_bwd (each writes one J*128-wide partial row)

// =====================================================================================
// Backward of the full-width edge term (fn_row_dots_sorted_f32 in fragnet_hip.hip is its forward)
// =====================================================================================
// g_feat[e,:] = sum_j g_s_sorted[inv(e), j] A[j];  part [grid, J*128]: partial sums of g_A[j,:] = sum_e g_s[e,j] feat[e,:]
struct RowDotsBwdArgs {
    const float *g_s_sorted, *feat, *A;
    int lda, off, J;
    fn_gat_plan pl;
    float* g_feat;
    float* part;
    const float* addend;
    int g_is_orig, nblk;
    // one-pass backward (gat_bwd_one.inc): g_feat rows are the finished gradient rows of the level whose RAW output is `feat`; their
    // dots c = <g, feat>, u = <g, out2> - c sigma are written with them (cu_c == null: not wanted; engine path with J = 4 heads only)
    const float *cu_out2, *cu_sigma;
    float *cu_c, *cu_u;
    const int32_t* n_real;   // nullable device word: edges (rows of feat) at or behind *n_real are padding: not read, not written
    int part_ld;             // layout of part (part_at, fn_internal.h): 0 = column-major [J * 128][FN_MAX_PART], else row-major [nblk][part_ld]
};
// edges [e0, e1) in original order, taken interleaved by the block's half-waves; vb: the block's slot (row) in T.part
__device__ __forceinline__ void row_dots_sorted_bwd_range(const RowDotsBwdArgs& T, float (*sR)[FN_D], int64_t e0, int64_t e1, int vb) {
    const float* __restrict__ g_s_sorted = T.g_s_sorted;
    const float* __restrict__ feat = T.feat;
    const float* __restrict__ A = T.A;
    const int lda = T.lda, off = T.off, J = T.J, g_is_orig = T.g_is_orig;
    const fn_gat_plan& pl = T.pl;
    float* g_feat = T.g_feat;
    float* __restrict__ part = T.part;
    const float* addend = T.addend;
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    float4 a[8], q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = (i < J) ? ld4(A + i * lda + off + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        q[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // rows are walked in original edge order (sequential feat / g_feat rows).  The per-head gradient comes either in
    // original order, edge-major [m_real][J] (written that way by the destination pass: one 16-byte read), or in
    // destination-sorted head-major order [J][m] through the inverse permutation (autograd path)
    if (g_is_orig && J == 4) {
        // engine path: 4 heads, gradient in original edge order.  Four rows per trip, every load issued before the
        // first use (a single-row loop is one dependent round trip per row: 15 us for 28 k rows)
        for (int64_t base = e0; base < e1; base += 4 * kRows) {
            float4 v[4], ad[4], gs[4], o2[4];
            float sgm[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                int64_t e = base + u * kRows + hw;
                e = e < e1 ? e : e1 - 1;
                v[u] = ld4(feat + e * FN_D + lane * 4);
                gs[u] = ld4(g_s_sorted + e * 4);
                ad[u] = addend ? ld4(addend + e * FN_D + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                o2[u] = (g_feat && T.cu_c && T.cu_out2) ? ld4(T.cu_out2 + e * FN_D + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                sgm[u] = (g_feat && T.cu_c && T.cu_out2) ? T.cu_sigma[e * 4 + (lane >> 3)] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t e = base + u * kRows + hw;
                if (e >= e1) continue;
                fma4(q[0], gs[u].x, v[u]);  fma4(q[1], gs[u].y, v[u]);  fma4(q[2], gs[u].z, v[u]);  fma4(q[3], gs[u].w, v[u]);
                if (!g_feat) continue;          // parameter partials only: the rows' term rides in a GEMM epilogue (RowAdd)
                float4 acc = ad[u];
                fma4(acc, gs[u].x, a[0]);  fma4(acc, gs[u].y, a[1]);  fma4(acc, gs[u].z, a[2]);  fma4(acc, gs[u].w, a[3]);
                st4(g_feat + e * FN_D + lane * 4, acc);
                if (T.cu_c) {            // four heads of eight lanes: the row's dots with its level's raw and second output rows
                    const float cc = head_sum<8>(dot4(acc, v[u])), uu = head_sum<8>(dot4(acc, o2[u]));
                    if ((lane & 7) == 0) {
                        const int64_t at = e * 4 + (lane >> 3);
                        T.cu_c[at] = cc;
                        if (T.cu_u) T.cu_u[at] = uu - cc * sgm[u];
                    }
                }
            }
        }
    } else
    for (int64_t e = e0 + hw; e < e1; e += kRows) {
        const size_t pos = g_is_orig ? 0 : (size_t)pl.inv_d[e];
        const float4 v = ld4(feat + e * FN_D + lane * 4);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < J) {
                const float gs = g_is_orig ? g_s_sorted[(size_t)e * J + i] : g_s_sorted[(size_t)i * pl.m + pos];
                fma4(acc, gs, a[i]);
                fma4(q[i], gs, v);
            }
        }
        if (addend) { const float4 a0 = ld4(addend + e * FN_D + lane * 4); acc.x += a0.x; acc.y += a0.y; acc.z += a0.z; acc.w += a0.w; }
        st4(g_feat + e * FN_D + lane * 4, acc);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < J) {                                    // J is a kernel argument: uniform branch
            st4(&sR[hw][lane * 4], q[i]);
            __syncthreads();
            if (threadIdx.x < FN_D) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < kRows; ++w) v += sR[w][threadIdx.x];
                part[part_at(T.part_ld, vb, i * FN_D + (int)threadIdx.x)] = v;
            }
            __syncthreads();
        }
    }
}
__device__ __forceinline__ void row_dots_sorted_bwd_body(const RowDotsBwdArgs& T, float (*sR)[FN_D], int vb, int nb) {
    // block_groups() for a virtual block index (the kernel may share its launch with another body)
    const int64_t m_live = T.n_real && *T.n_real < T.pl.m_real ? (int64_t)*T.n_real : T.pl.m_real;
    const int64_t groups = (T.pl.m_real + kRows - 1) / kRows, per = (groups + nb - 1) / nb;
    const int64_t live_blocks = (m_live + per * kRows - 1) / (per * kRows);
    const int64_t g0 = (int64_t)xcd_block_real(vb, nb, (int)(live_blocks < nb ? live_blocks : nb)) * per, g1 = g0 + per < groups ? g0 + per : groups;
    const int64_t e1 = g1 * kRows < m_live ? g1 * kRows : m_live;
    row_dots_sorted_bwd_range(T, sR, g0 * kRows < e1 ? g0 * kRows : e1, e1, vb);
}
__global__ __launch_bounds__(kBlock) void k_row_dots_sorted_bwd(RowDotsBwdArgs T) {
    __shared__ float sR[kRows][FN_D];
    row_dots_sorted_bwd_body(T, sR, (int)blockIdx.x, (int)gridDim.x);
}
// The source pass of a level and the backward of its edge term both depend on the destination pass only, never on each
// other: one launch (a dependent launch costs ~5 us however small the kernel is; 5 such pairs per backward pass).
template <int H, int RB>
__global__ __launch_bounds__(RB * 32) void k_gat_bwd_src_rd(GatBwdSrcArgs A, RowDotsBwdArgs T) {
    static_assert(RB * 32 == kBlock && RB == kRows, "both bodies run 8 half-waves per block");
    __shared__ float sA[RB][2 * FN_D];
    if ((int)blockIdx.x < A.nblk) gat_bwd_src_body<H, RB>(A, sA, (int)blockIdx.x, A.nblk);
    else row_dots_sorted_bwd_body(T, reinterpret_cast<float(*)[FN_D]>(&sA[0][0]), (int)blockIdx.x - A.nblk, T.nblk);
}

// Last layer's fragment tail, first half, as ONE launch: blocks [0, nblk_seg) = the atom -> fragment sum (block_rows_sum, the body of
// k_segment_sum128_wide) followed by the fragment's node scalars <row, att[h, dst/src block]> from the finished row (a head's
// 128/H columns are consecutive threads: shuffle reduction) -- two launches less than sum, node scalars, edge term; blocks
// [nblk_seg, +nblk_rd) = the fragment graph's edge term <new_fbond[e], att[h, mid block]> (row_dots_sorted_body, the body of
// k_row_dots_sorted), which depends on neither.  Each of the three was a ~5 us latency-floor launch.
struct FragTailArgs {
    const float* src;  const int32_t* rowptr;  const int32_t* perm;  int32_t pos_base;  float* out;  int64_t n_seg;
    const float* att;  int att_w, dst_off, src_off;  float* s_dst;  float* s_src;  int nblk_seg;
    const float* feat;  const float* A;  int lda, off;  fn_gat_plan pl;  float* s_sorted;  int nblk_rd;
};
template <int H>
__global__ __launch_bounds__(kBlock) void k_frag_tail(FragTailArgs T) {
    __shared__ float sS[kRows][FN_D];
    if ((int)blockIdx.x >= T.nblk_seg) {
        row_dots_sorted_body<H>(T.feat, T.A, T.lda, T.off, H, T.pl, T.s_sorted, (int)blockIdx.x - T.nblk_seg, T.nblk_rd);
        return;
    }
    constexpr int d = FN_D / H;
    static_assert(d <= 64, "a head's columns must lie inside one wave");
    const int t = threadIdx.x, head = (t & 127) / d, c = (t & 127) % d;
    const float a_d = T.att[head * T.att_w + T.dst_off + c], a_s = T.att[head * T.att_w + T.src_off + c];
    for (int64_t s = blockIdx.x; s < T.n_seg; s += T.nblk_seg) {
        float v = 0.f;                                       // the column sum, taken out: the node scalars need waves 0 and 1 whole
        block_rows_sum(sS, T.src, FN_D, T.perm, T.rowptr[s] - T.pos_base, T.rowptr[s + 1] - T.rowptr[s], KeepAllRows{}, [&](float x) { v = x; });
        if (t < FN_D) {
            T.out[s * FN_D + t] = v;
            float pd = v * a_d, ps = v * a_s;
#pragma unroll
            for (int off = d / 2; off > 0; off >>= 1) { pd += __shfl_xor(pd, off);  ps += __shfl_xor(ps, off); }
            if (c == 0) { T.s_dst[s * H + head] = pd;  T.s_src[s * H + head] = ps; }
        }
        __syncthreads();
    }
}

// g_x = (y > 0) ? g_y * scale : 0 for up to four tensors (numel % 4 == 0, 16-byte aligned) in one launch
struct GateTask {
    const float *g, *y;
    float* o;
    int64_t n4;
    int first, nblk;
};
struct GateTasks {
    GateTask t[4];
    int n, blocks;
    float scale;
};
__global__ void k_gate_many(GateTasks G) {
    int ti = 0;
    while (ti + 1 < G.n && (int)blockIdx.x >= G.t[ti + 1].first) ++ti;
    const GateTask& t = G.t[ti];
    const float sc = G.scale;
    for (int64_t i = (int64_t)((int)blockIdx.x - t.first) * blockDim.x + threadIdx.x; i < t.n4; i += (int64_t)t.nblk * blockDim.x) {
        const float4 g = ld4(t.g + 4 * i), v = ld4(t.y + 4 * i);
        st4(t.o + 4 * i, make_float4(v.x > 0.f ? g.x * sc : 0.f, v.y > 0.f ? g.y * sc : 0.f, v.z > 0.f ? g.z * sc : 0.f,
                                     v.w > 0.f ? g.w * sc : 0.f));
    }
}

#include "linear128.inc"

// the one-pass backward's second launch of a layer: input-gradient products (one 64 x 64 tile per workgroup; RowAdd epilogue where a
// task carries one; the epilogue also writes the dots c = <g, out>, u = <g, out2> - c sigma of the rows it finishes, CuEpi)  ||  the
// parameter-gradient partials of the atom graph's edge term
__global__ __launch_bounds__(kBlock, 3) void k_lin_rd_cu(LinTasks T, RowDotsBwdArgs R) {
    extern __shared__ __attribute__((aligned(16))) float sBt[];
    __shared__ float sR[kRows][FN_D];
    const int b = (int)blockIdx.x;
    if (b < T.total) { lin_side_block<true>(sBt, T, b);  return; }
    row_dots_sorted_bwd_body(R, sR, b - T.total, R.nblk);
}

// x_sorted[pos, :] = x[eid(pos), :] (zeros at loop positions): raw edge attributes are permuted once per batch
__device__ __forceinline__ void sort_edge_attr_body(const float* __restrict__ x, int K, const fn_gat_plan& pl,
                                                    float* __restrict__ x_sorted, int vb, int nb) {
    const int64_t total = pl.m * K;
    for (int64_t i = (int64_t)vb * blockDim.x + threadIdx.x; i < total; i += (int64_t)nb * blockDim.x) {
        const int64_t pos = i / K;
        const int k = (int)(i % K);
        const int eid = pl.eid_d[pos];
        x_sorted[(size_t)k * pl.m + pos] = eid < pl.m_real ? x[(size_t)eid * K + k] : 0.f;   // [K][m]
    }
}
// the same attribute in SOURCE order (x_src[:, q] = the attribute of the edge at source-order position q): the one-pass backward
// streams it; x_raw != null: from the original edge order ([m_real][K]), else from the destination-sorted copy ([K][m])
__device__ __forceinline__ void sort_edge_attr_src_body(const float* __restrict__ x_raw, const float* __restrict__ x_sorted, int K,
                                                        const fn_gat_plan& pl, float* __restrict__ x_src, int vb, int nb) {
    const int64_t total = pl.m * K;
    for (int64_t i = (int64_t)vb * blockDim.x + threadIdx.x; i < total; i += (int64_t)nb * blockDim.x) {
        const int64_t pos = i / K;
        const int k = (int)(i % K);
        const int dq = pl.dpos_s[pos];
        float v;
        if (x_raw) { const int eid = pl.eid_d[dq];  v = eid < pl.m_real ? x_raw[(size_t)eid * K + k] : 0.f; }
        else v = x_sorted[(size_t)k * pl.m + dq];
        x_src[(size_t)k * pl.m + pos] = v;
    }
}
__global__ void k_sort_edge_attr(const float* __restrict__ x, int K, fn_gat_plan pl, float* __restrict__ x_sorted, int by_source) {
    if (by_source) sort_edge_attr_src_body(x, nullptr, K, pl, x_sorted, (int)blockIdx.x, (int)gridDim.x);
    else sort_edge_attr_body(x, K, pl, x_sorted, (int)blockIdx.x, (int)gridDim.x);
}

// all projection weights of the encoder, transposed by the forward prologue's first block range: matrix z -> Bt base + z * 192 * 128
struct TransposeMany {
    const float* W[3 * FN_MAX_LAYERS];
    int K[3 * FN_MAX_LAYERS];
};
__device__ __forceinline__ void transpose_many_body(const TransposeMany& tm, float* __restrict__ bt_base, float (*tile)[33],
                                                    int z, int by, int bx) {
    const int K = tm.K[z];
    const int k0 = bx * 32, n0 = by * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (k0 >= K) return;                                            // whole block
    const float* W = tm.W[z];
    float* Bt = bt_base + (size_t)z * 192 * FN_D;
    for (int r = ty; r < 32; r += 8) tile[r][tx] = (k0 + tx < K) ? W[(size_t)(n0 + r) * K + k0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (k0 + r < K) Bt[(size_t)(k0 + r) * FN_D + n0 + tx] = tile[tx][r];
}

// extents of every molecule in the index spaces of a collated batch (fn_internal.h: MolExt), from the molecule CSRs and the level plans
using fni::MolExt;
struct MolExtArgs {
    const int32_t *mol_atoms, *mol_frags;       // molecule CSRs over atoms / fragments (global positions)
    int32_t base_atoms, base_frags;
    fn_gat_plan bond, atom, fbond, frag;
    int n_mol;
    MolExt* out;
    const int32_t* counts_dev;                  // nullable: device count of the real molecules (the rest is padding)
    int32_t* real_rows;                         // nullable: [4] real atoms / bonds / fragments / connections = where the last real molecule ends
};
__device__ __forceinline__ void mol_extents_body(const MolExtArgs& A, int vb) {
    const int mol = vb * blockDim.x + threadIdx.x;
    if (mol >= A.n_mol) return;
    MolExt x;
    const int a0 = A.mol_atoms[mol] - A.base_atoms, a1 = A.mol_atoms[mol + 1] - A.base_atoms;
    const int f0 = A.mol_frags[mol] - A.base_frags, f1 = A.mol_frags[mol + 1] - A.base_frags;
    // the by-source CSR of the atom graph counts, before atom a, the bonds leaving atoms < a (+ one loop item per atom)
    const int la = A.atom.m > A.atom.m_real ? 1 : 0, lf = A.frag.m > A.frag.m_real ? 1 : 0;
    const int b0 = A.atom.rowptr_s[a0] - A.atom.pos_base_s - la * a0, b1 = A.atom.rowptr_s[a1] - A.atom.pos_base_s - la * a1;
    const int c0 = A.frag.rowptr_s[f0] - A.frag.pos_base_s - lf * f0, c1 = A.frag.rowptr_s[f1] - A.frag.pos_base_s - lf * f1;
    x.a0 = a0;  x.na = a1 - a0;  x.b0 = b0;  x.nb = b1 - b0;  x.f0 = f0;  x.nf = f1 - f0;  x.c0 = c0;  x.nc = c1 - c0;
    x.eb0 = A.bond.rowptr_d[b0] - A.bond.pos_base_d;   x.meb = A.bond.rowptr_d[b1] - A.bond.pos_base_d - x.eb0;
    x.ea0 = A.atom.rowptr_d[a0] - A.atom.pos_base_d;   x.mea = A.atom.rowptr_d[a1] - A.atom.pos_base_d - x.ea0;
    if (A.fbond.rowptr_d) {
        x.ef0 = A.fbond.rowptr_d[c0] - A.fbond.pos_base_d;  x.mef = A.fbond.rowptr_d[c1] - A.fbond.pos_base_d - x.ef0;
    } else { x.ef0 = 0;  x.mef = 0; }
    x.ec0 = A.frag.rowptr_d[f0] - A.frag.pos_base_d;   x.mec = A.frag.rowptr_d[f1] - A.frag.pos_base_d - x.ec0;
    A.out[mol] = x;
    if (A.real_rows) {
        int n_real = A.counts_dev ? *A.counts_dev : A.n_mol;
        n_real = n_real < A.n_mol ? n_real : A.n_mol;
        if (mol == n_real - 1) { A.real_rows[0] = a1;  A.real_rows[1] = b1;  A.real_rows[2] = f1;  A.real_rows[3] = c1; }
        if (n_real <= 0 && mol == 0) { A.real_rows[0] = 0;  A.real_rows[1] = 0;  A.real_rows[2] = 0;  A.real_rows[3] = 0; }
    }
}
#include "mol_tail.inc"

// Everything the encoder's forward pass needs before its first projection, none of which depends on the other: W^T of
// every projection, dropout of the atom features, and the permutation of the two raw edge-attribute tensors into
// destination order.  One launch of four block ranges instead of four launches (each was 5 us of latency).
struct EncPrologue {
    TransposeMany tm;
    float* bt_base;
    int n_t;                                                        // 24 blocks per matrix
    const float* dx;  float* dy;  int64_t dnumel;  float p;  uint64_t seed, offset;  const uint64_t* offset_dev;  int n_d;
    const uint8_t* dgate;  int dgate_w;                             // fn_encoder_forward_keep: the input gate of x_atoms (null: none), one byte per dgate_w elements
    const float* sx[2];  float* so[2];  int sK[2];  fn_gat_plan spl[2];  int n_s[2];
    const float* ssr[2];  const float* sss[2];  float* sso[2];  int n_ss[2];   // the same two attributes in SOURCE order (one-pass backward): from raw, else from sorted
    float* zp;  int64_t zn;  int n_z;                               // buffer zeroed once per forward (edge-term scratch: loop positions stay 0)
    MolExtArgs mx;  int n_x;                                        // molecule extents for the molecule-resident backward (256 molecules per block)
};
// GATED: the gated pass's instance (fn_encoder_forward_keep).  An instance of its own, so that the plain pass's dropout range carries no
// test of the gate pointer
template <bool GATED>
__global__ __launch_bounds__(256) void k_enc_prologue(EncPrologue A) {
    __shared__ float tile[32][33];
    int b = blockIdx.x;
    if (b < A.n_t) {
        const int z = b / 24, rem = b % 24;
        transpose_many_body(A.tm, A.bt_base, tile, z, rem / 6, rem % 6);
        return;
    }
    b -= A.n_t;
    if (b < A.n_d) {
        if (GATED) dropout_act_body<false>(A.dx, nullptr, A.dy, A.dnumel, A.p, A.seed, A.offset, A.offset_dev, 0, b, A.n_d, A.dgate, A.dgate_w);
        else dropout_act_body<false>(A.dx, nullptr, A.dy, A.dnumel, A.p, A.seed, A.offset, A.offset_dev, 0, b, A.n_d);
        return;
    }
    b -= A.n_d;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (b < A.n_s[q]) {
            sort_edge_attr_body(A.sx[q], A.sK[q], A.spl[q], A.so[q], b, A.n_s[q]);
            return;
        }
        b -= A.n_s[q];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        if (b < A.n_ss[q]) {
            sort_edge_attr_src_body(A.ssr[q], A.sss[q], A.sK[q], A.spl[q], A.sso[q], b, A.n_ss[q]);
            return;
        }
        b -= A.n_ss[q];
    }
    if (b < A.n_z) {
        for (int64_t i = (int64_t)b * blockDim.x + threadIdx.x; i < A.zn; i += (int64_t)A.n_z * blockDim.x) A.zp[i] = 0.f;
        return;
    }
    b -= A.n_z;
    if (b < A.n_x) mol_extents_body(A.mx, b);
}

}  // namespace

// =====================================================================================
// Encoder engine: FragNet.forward / its backward as ONE call each (reference gat2.py:381-442 and, per layer,
// gat2.py:121-330).  The host only walks the layer list and enqueues kernels on the caller's stream; nothing is
// allocated, nothing synchronises.  Activations the backward pass needs live in the caller's workspace.
// =====================================================================================
namespace {

struct Bump {
    float* base;
    int64_t used = 0;
    explicit Bump(float* b) : base(b) {}
    float* take(int64_t n) {
        float* p = base ? base + used : nullptr;
        used += (n + 63) / 64 * 64;          // 256-byte granules keep every buffer 16-byte aligned
        return p;
    }
};

// The three projected attention levels of a layer.  The value is the level's slot in the per-layer tables of the workspace: the
// transposed projection weights (EncLayout::bt) of layer l's level v are entry 3 l + v.  The fragment graph is a fourth level without
// a projection (no slot); only the last layer's ever runs.
enum Level : int { LV_BOND = 0, LV_ATOM = 1, LV_FBOND = 2, LV_FRAG = 3 };
constexpr int kLevels = 3;
constexpr Level kProjected[kLevels] = {LV_BOND, LV_ATOM, LV_FBOND};
inline int64_t level_rows(const fn_encoder* e, Level v) { return v == LV_BOND ? e->E : v == LV_ATOM ? e->N : v == LV_FBOND ? e->EF : e->F; }
inline const fn_gat_plan& level_plan(const fn_encoder* e, Level v) { return v == LV_BOND ? e->bond : v == LV_ATOM ? e->atom : v == LV_FBOND ? e->fbond : e->frag; }
inline int level_k0(const fn_encoder* e, Level v) { return v == LV_BOND ? e->k_bond0 : v == LV_ATOM ? e->k_atom0 : v == LV_FBOND ? e->k_fbond0 : 0; }

struct LevelActs {           // a level's rows, kept from forward for backward
    float *h, *raw, *p;      // projected rows (fragment graph: the fragment sums), raw output rows (atom level: EncLayout::atoms_new, one
                             // buffer for all layers; fragment graph: none), probabilities
    float* y;                // post dropout+ReLU output (null for the last layer: caller's buffers)
    float *o2, *sg;          // one-pass backward (FN_TUNE_BWD_ONE, training): the forward's second output rows and their weight sums
};
struct LayerActs {
    LevelActs lv[kLevels + 1];       // by Level
};

struct EncLayout {
    LayerActs L[FN_MAX_LAYERS];
    float* in_atoms0;        // dropout(x_atoms) when training with p > 0 or gate(x_atoms) of a gated pass, else null (use x_atoms)
    // forward scratch (s_dst / s_src: a level's node scalars; the bond level's pair is sized for the largest index space and also
    // serves the fragment graph, which runs when the bond level is done)
    float *atoms_new, *frags_new, *s_sorted, *s_dst[kLevels], *s_src[kLevels], *bt;
    float* mol_ext;          // MolExt[n_mols] for the molecule-resident backward (null without molecule CSRs)
    float *xs_bond, *xs_fbond;   // one-pass backward: the two raw edge attributes in source order ([1][bond.m], [k_fattr][fbond.m])
    float* real_rows;            // pad_skip_on: int32 [4] = real atoms, bonds, fragments, connections (written by the forward prologue)
    int64_t total;
};

inline int64_t max4(int64_t a, int64_t b, int64_t c, int64_t d) { return std::max(std::max(a, b), std::max(c, d)); }

// every attention level's backward as one source-owner pass (csrc/gat_bwd_one.inc).  Decided from the descriptor and the
// process-wide tuning table alone, so that fn_encoder_forward (which then writes out2 / sigma), fn_encoder_backward and the
// workspace sizes agree; gat2_edge's fragment graph (edge class FN_MAX_EDGE_K on 128-wide embeddings) keeps the two passes
bool one_pass_on(const fn_encoder* e);
// Padding rows of a static-shape batch are skipped by the kernels of the one-pass path: the rows behind the real ones in every index
// space (collate appends the padding molecules) get zero outputs / zero gradients without gathers or matrix work, GEMM tiles and
// weight-gradient rows beyond them are not touched.  Needs the molecule CSRs (the real counts are the extents of the last real
// molecule, written by the forward prologue) and the device count of real molecules.
bool pad_skip_on(const fn_encoder* e);
bool one_pass_on(const fn_encoder* e) {
    return tune(FN_TUNE_BWD_ONE) != 0 && e->training != 0 && (e->heads == 2 || e->heads == 4 || e->heads == 8) &&
           e->atom.m_real == e->E;
}

// The form a forward pass ran in (1: one-pass backward = out2 / sigma exist; 0: two passes), latched per activation workspace:
// fn_encoder_backward refuses a descriptor whose form -- read from the process-wide tuning table -- is no longer the one its forward
// wrote the workspace in (FN_TUNE_BWD_ONE flipped in between would leave out2 / sigma null or unwritten for the other half).
int enc_form(const fn_encoder* e) { return one_pass_on(e) ? 1 : 0; }
struct FormLatch { const float* ws; int form; bool gated; };     // gated: the forward ran with an input gate (fn_encoder_forward_keep)
FormLatch g_form_latch[64];
int g_form_latch_next = 0;
std::mutex g_form_latch_mu;
void latch_form(const fn_encoder* e, bool gated) {
    std::lock_guard<std::mutex> lk(g_form_latch_mu);
    for (FormLatch& f : g_form_latch)
        if (f.ws == e->ws) { f.form = enc_form(e);  f.gated = gated;  return; }
    g_form_latch[g_form_latch_next] = FormLatch{e->ws, enc_form(e), gated};
    g_form_latch_next = (g_form_latch_next + 1) % 64;
}
bool form_matches_forward(const fn_encoder* e) {      // (a workspace this process ran no forward into: nothing to compare with)
    std::lock_guard<std::mutex> lk(g_form_latch_mu);
    for (const FormLatch& f : g_form_latch)
        if (f.ws == e->ws && f.ws) return f.form == enc_form(e);
    return true;
}
// did the last forward pass into this workspace run with an input gate?  Its backward then reads the gated copy of x_atoms, which
// with p_eff == 0 lives behind the plain workspace (enc_layout's `gated`)
bool forward_was_gated(const fn_encoder* e) {
    std::lock_guard<std::mutex> lk(g_form_latch_mu);
    for (const FormLatch& f : g_form_latch)
        if (f.ws == e->ws && f.ws) return f.gated;
    return false;
}

EncLayout enc_layout(const fn_encoder* e, float* ws, bool gated = false) {
    EncLayout o{};
    Bump b(ws);
    const int H = e->heads;
    const bool drop = e->training && e->drop_p > 0.f;
    for (int l = 0; l < e->n_layers; ++l) {
        LayerActs& a = o.L[l];
        for (Level v : kProjected) a.lv[v].h = b.take(level_rows(e, v) * FN_D);
        a.lv[LV_FRAG].h = b.take(e->F * FN_D);
        a.lv[LV_BOND].raw = b.take(e->E * FN_D);  a.lv[LV_FBOND].raw = b.take(e->EF * FN_D);
        for (Level v : kProjected) a.lv[v].p = b.take(level_plan(e, v).m * H);
        a.lv[LV_FRAG].p = b.take(e->frag.m * H);
        if (l + 1 < e->n_layers) {
            a.lv[LV_ATOM].y = b.take(e->N * FN_D);  a.lv[LV_FRAG].y = b.take(e->F * FN_D);
            a.lv[LV_BOND].y = b.take(e->E * FN_D);  a.lv[LV_FBOND].y = b.take(e->EF * FN_D);
        }
    }
    if (one_pass_on(e)) {
        for (int l = 0; l < e->n_layers; ++l) {
            LayerActs& a = o.L[l];
            for (Level v : kProjected) a.lv[v].o2 = b.take(level_rows(e, v) * FN_D);
            for (Level v : kProjected) a.lv[v].sg = b.take(level_rows(e, v) * H);
        }
        o.xs_bond = b.take(e->bond.m);
        o.xs_fbond = b.take(e->fbond.m * e->k_fattr);
    }
    o.real_rows = pad_skip_on(e) ? b.take(64) : nullptr;
    o.in_atoms0 = drop ? b.take(e->N * e->k_atom0) : nullptr;
    o.atoms_new = b.take(e->N * FN_D);
    for (int l = 0; l < e->n_layers; ++l) o.L[l].lv[LV_ATOM].raw = o.atoms_new;
    o.frags_new = b.take(e->F * FN_D);
    o.s_sorted = b.take(std::max(e->atom.m, e->frag.m) * H);
    const int64_t nmax = max4(e->E, e->N, e->EF, e->F);
    for (Level v : kProjected) {
        const int64_t n = v == LV_BOND ? nmax : level_rows(e, v);
        o.s_dst[v] = b.take(n * H);
        o.s_src[v] = b.take(n * H);
    }
    o.bt = b.take((int64_t)3 * e->n_layers * 192 * FN_D);
    o.mol_ext = e->n_mols > 0 ? b.take(e->n_mols * (int64_t)(sizeof(MolExt) / sizeof(float))) : nullptr;
    // a gated pass without dropout keeps its gated copy of x_atoms behind everything else: no other offset moves
    if (gated && !drop) o.in_atoms0 = b.take(e->N * e->k_atom0);
    o.total = b.used;
    return o;
}

bool have_mol(const fn_encoder* e) {       // the caller handed over the molecule CSRs: every level is block-diagonal per molecule
    return e->n_mols > 0 && e->mol_atoms.rowptr && e->mol_frags.rowptr && e->mol_atoms.n_seg == e->n_mols && e->mol_frags.n_seg == e->n_mols;
}
bool pad_skip_on(const fn_encoder* e) {
    return tune(FN_TUNE_PAD_SKIP) != 0 && one_pass_on(e) && have_mol(e) && e->mol_contiguous != 0 && e->counts_dev != nullptr && e->variant == 0;
}
// the last layer's fragment tail (fragment sums -> fragment graph -> readout, and its backward) as one molecule-resident launch
// each way (csrc/mol_tail.inc): needs the caller's word that the batch has collate_fn's molecule-contiguous layout
bool tail_mol_on(const fn_encoder* e) {
    return tune(FN_TUNE_MOL_TAIL) != 0 && e->mol_contiguous != 0 && have_mol(e) && e->variant == 0 &&
           (e->heads == 2 || e->heads == 4 || e->heads == 8) && e->F > 0 && e->EF > 0 && e->frag.m > 1 && e->n_mols <= FN_MAX_PART &&
           !((uintptr_t)e->ws & 15);
}

// Backward scratch.  Nothing is reused across levels or layers: the kernels that only produce parameter gradients
// (finalize, weight-gradient GEMMs, column sums) run on an auxiliary stream behind the main dependency chain, so a
// buffer they read must not be rewritten by the next level.  ~60 MB per layer at ESOL batch 512.
// part_a / part_rd: one row of partial sums per block, row-major [FN_MAX_PART][256] / [FN_MAX_PART][H * 128] (part_at, fn_internal.h; the
// same floats as the column-major form the operator entry points keep).  EVERY engine launch that writes one of them and every task that
// reduces one takes its layout from the two functions below.
constexpr int part_a_ld() { return FN_PART_ROWMAJOR ? 2 * FN_D : 0; }
constexpr int part_rd_ld(int H) { return FN_PART_ROWMAJOR ? H * FN_D : 0; }
struct LevelScratch {
    float *g_h, *dz, *pz, *g_s_dst, *part_a, *part_e, *part_rd, *wg_ws;
    float* cdot;             // one-pass backward: c[n, H] = <g, out> per head (no pz then)
};
struct BwdLayout {
    float* g_pre[kLevels + 1];   // by Level: grads w.r.t. pre-activation layer outputs (the chain)
    float* g_frags;
    LevelScratch lv[FN_MAX_LAYERS][kLevels], frag;
    int64_t total;
};

BwdLayout bwd_layout(const fn_encoder* e, float* ws) {
    BwdLayout o{};
    Bump b(ws);
    const int H = e->heads;
    o.g_pre[LV_ATOM] = b.take(e->N * FN_D);  o.g_pre[LV_FRAG] = b.take(e->F * FN_D);
    o.g_pre[LV_BOND] = b.take(e->E * FN_D);  o.g_pre[LV_FBOND] = b.take(e->EF * FN_D);
    o.g_frags = b.take(e->F * FN_D);
    auto level = [&](LevelScratch& s, int64_t n, int64_t m, int k0, bool edge_params, bool row_dots, bool proj, bool one = false) {
        s.g_h = b.take(n * FN_D);
        s.dz = row_dots ? b.take(m * H) : nullptr;
        s.pz = one ? nullptr : b.take(2 * m * H);
        s.cdot = one ? b.take(n * H) : nullptr;
        s.g_s_dst = b.take(n * H);
        s.part_a = b.take((int64_t)FN_MAX_PART * 2 * FN_D);
        s.part_e = edge_params ? b.take((int64_t)FN_MAX_PART * H * (FN_MAX_EDGE_K + 1)) : nullptr;
        s.part_rd = row_dots ? b.take((int64_t)FN_MAX_PART * H * FN_D) : nullptr;
        s.wg_ws = proj ? b.take(fn_linear128_wgrad_ws(n, k0 > FN_D ? k0 : FN_D)) : nullptr;
    };
    // the atom level's edge term is a table of row dots (parameter partials part_rd); the other two embed a raw attribute (part_e)
    for (int l = 0; l < e->n_layers; ++l)
        for (Level v : kProjected)
            level(o.lv[l][v], level_rows(e, v), level_plan(e, v).m, level_k0(e, v), v != LV_ATOM, v == LV_ATOM, true, one_pass_on(e));
    level(o.frag, e->F, e->frag.m, 0, e->variant == 2, true, false);      // gat2_edge: the fragment graph has edge-embedding partials
    o.total = b.used;
    return o;
}

inline uint64_t blocks4(int64_t numel) { return (uint64_t)((numel + 3) / 4); }

// Philox offsets consumed by the encoder, in order: input dropout of x_atoms, then per layer atoms, frags, bond, fbond
struct RngPlan {
    uint64_t in_atoms;
    uint64_t y[FN_MAX_LAYERS][4];
    uint64_t total;
};
RngPlan rng_plan(const fn_encoder* e) {
    RngPlan r{};
    uint64_t off = e->offset;
    r.in_atoms = off;  off += blocks4(e->N * e->k_atom0);
    for (int l = 0; l < e->n_layers; ++l) {
        r.y[l][0] = off;  off += blocks4(e->N * FN_D);
        r.y[l][1] = off;  off += blocks4(e->F * FN_D);
        r.y[l][2] = off;  off += blocks4(e->E * FN_D);
        r.y[l][3] = off;  off += blocks4(e->EF * FN_D);
    }
    r.total = off - e->offset;
    return r;
}

// ---- the level view: everything the passes need to know about one attention level of one layer, described ONCE.  A plain struct on
// the stack, built where a level is used; the forward, both backward forms and the parameter work all read the same description.
struct LevelWeights {        // a level's parameters inside a fn_layer_weights (the engine's, or the caller's gradient block)
    float *att, *W, *bias, *embW, *embb;      // attention vector, projection, edge-attribute embedding (null: the level has none)
};
inline LevelWeights level_weights(const fn_layer_weights& w, Level v, int variant = 0) {
    switch (v) {
        case LV_BOND: return {w.a_b, w.proj_b_w, w.proj_b_b, w.emb_b_w, w.emb_b_b};
        case LV_ATOM: return {w.a, w.proj_a_w, w.proj_a_b, nullptr, nullptr};
        case LV_FBOND: return {w.f_a_b, w.proj_fb_w, w.proj_fb_b, w.emb_fb_w, w.emb_fb_b};
        default: break;
    }
    // the fragment graph: gat2_edge embeds the connection attribute there (with the fragment-bond level's Linear, which it does not run)
    return {w.f, nullptr, nullptr, variant == 2 ? w.emb_fb_w : nullptr, variant == 2 ? w.emb_fb_b : nullptr};
}
struct LevelView {
    Level lv;  int layer, H;
    const fn_gat_plan* pl;  int64_t rows;
    // attention vector [H][att_w]: destination block at 0, source block at src_off; mid_off: the block of the edge term (bond /
    // fragment-bond level: the embedded attribute's, d wide; atom level / fragment graph: dotted with the raw bond / fragment-bond rows)
    const float* att;  int att_w, src_off, mid_off;
    const float *W, *bias, *Wt;     // projection [128][K], its bias, the transposed copy the forward prologue leaves in the workspace
    const float* x;  int K;         // the projection's input rows: the level's activated output of the layer below, raw features (K wide) at layer 0
    // edge term as the attention kernels take it (x_src: the source-order attribute table of the one-pass backward, null otherwise).
    // Atom level and gat2's fragment graph: mode 0, a table of row dots; the forward points s_sorted at the table it fills
    fn_edge_term et;
    const int32_t* n_real;          // pad_skip_on: device word, rows at or behind it are padding; else null
    float *s_dst, *s_src;           // node-scalar scratch of the forward
    LevelActs a;                    // what the forward keeps of the level
    int rng_slot;                   // RngPlan::y[layer][.]: ordered atoms, frags, bond, fbond -- NOT the Level order
};
LevelView level_view(const fn_encoder* e, const EncLayout& lay, int l, Level v) {
    const int d = FN_D / e->heads;
    const LevelWeights w = level_weights(e->w[l], v, e->variant);
    const int32_t* rr = reinterpret_cast<const int32_t*>(lay.real_rows);       // (null unless pad_skip_on: enc_layout)
    LevelView o{};
    o.lv = v;  o.layer = l;  o.H = e->heads;
    o.pl = &level_plan(e, v);  o.rows = level_rows(e, v);
    o.att = w.att;
    o.a = lay.L[l].lv[v];
    if (v == LV_BOND || v == LV_FBOND) { o.att_w = 3 * d;  o.src_off = 2 * d; }
    else { o.att_w = 2 * d + FN_D;  o.src_off = d + FN_D; }
    o.mid_off = d;
    if (v != LV_FRAG) {
        o.W = w.W;  o.bias = w.bias;  o.K = l ? FN_D : level_k0(e, v);
        o.Wt = lay.bt + (size_t)(3 * l + v) * 192 * FN_D;
        o.s_dst = lay.s_dst[v];  o.s_src = lay.s_src[v];
    } else { o.s_dst = lay.s_dst[LV_BOND];  o.s_src = lay.s_src[LV_BOND]; }
    switch (v) {
        case LV_BOND:
            o.x = l ? lay.L[l - 1].lv[v].y : e->bond_nodes;
            o.et = fn_edge_term{2, 1, d, d, nullptr, e->cos_sorted, w.embW, w.embb, lay.xs_bond};
            o.n_real = rr ? rr + 1 : nullptr;  o.rng_slot = 2;
            break;
        case LV_ATOM:
            o.x = l ? lay.L[l - 1].lv[v].y : (lay.in_atoms0 ? lay.in_atoms0 : e->x_atoms);
            o.n_real = rr;  o.rng_slot = 0;
            break;
        case LV_FBOND:
            o.x = l ? lay.L[l - 1].lv[v].y : e->fbond_nodes;
            o.et = fn_edge_term{2, e->k_fattr, d, d, nullptr, e->fattr_sorted, w.embW, w.embb, lay.xs_fbond};
            o.n_real = rr ? rr + 3 : nullptr;  o.rng_slot = 3;
            break;
        case LV_FRAG:        // gat2_edge: the connection attribute rides on the fragment graph's edges, embedded 128 wide
            if (e->variant == 2) o.et = fn_edge_term{2, e->k_fattr, FN_D, d, nullptr, e->fattr_sorted, w.embW, w.embb, nullptr};
            o.n_real = rr ? rr + 2 : nullptr;  o.rng_slot = 1;
            break;
    }
    return o;
}
// the act(dropout(.)) epilogue that writes (forward) or replays (backward: the gate of an input-gradient product) the level's output y
inline fn_act_epilogue act_epilogue(const fn_encoder* e, const RngPlan& rng, const LevelView& v, float* y) {
    return fn_act_epilogue{y, e->training ? e->drop_p : 0.f, 1, e->seed, rng.y[v.layer][v.rng_slot], e->offset_dev};
}
// dL/d(relu(dropout(x))) = gate_scale * dL/dy where y > 0
inline float gate_scale(const fn_encoder* e) {
    const float p = e->training ? e->drop_p : 0.f;
    return p > 0.f ? (p < 1.f ? 1.f / (1.f - p) : 0.f) : 1.f;
}
// the four outputs of the encoder, or the gradients w.r.t. them, by Level (null: not stored / zero)
struct EncOutputs { const float* y[kLevels + 1]; };

// the level's edge term as the forward's attention kernels take it (mode 0: the table of row dots the forward fills)
inline fn_edge_term fwd_edge_term(const LevelView& v, const float* s_sorted) {
    fn_edge_term et = v.et;
    et.x_src = nullptr;
    if (et.mode == 0) et.s_sorted = s_sorted;
    return et;
}
// the node scalars <h[row, head], att dst / src block> of a level, as the epilogue of its projection
inline NodeScalarEpi node_scalars(const LevelView& v) { return NodeScalarEpi{v.att, v.s_dst, v.s_src, v.att_w, 0, v.src_off, v.H}; }
// the level's projection h = x W^T + b (+ node scalars) as a task of a grouped launch.  k_task != 0: a launch whose tasks have
// reduction lengths of their own (layer 0's raw features)
inline LinTask proj_task(const LevelView& v, int k_task = 0) {
    LinTask t{v.W, v.x, v.Wt, v.bias, v.a.h, v.rows, fn_act_epilogue{nullptr, 0.f, 0, 0, 0, nullptr}, node_scalars(v), 0, 0, k_task};
    t.n_real = v.n_real;
    return t;
}

// a level's parameter work: the attention vector's and edge embedding's gradients from the partial rows its pass wrote (n_a, n_e),
// and the projection's weight gradient from its g_h rows
struct ParamWork {
    int n_a = 0, n_e = 0;
    int n_rd = 0;                    // two-pass atom level: partial rows of the edge term's dL/da[:, mid block], reduced between the two
};
// ... as the parameter-gradient queue (param_grads.hip) takes it: the level's description unpacked into pointers and counts
inline fni::AttParamGrads att_param_grads(const LevelView& v, const LevelWeights& g, const LevelScratch& sc, int n_a, int n_e) {
    return fni::AttParamGrads{v.H, sc.part_a, n_a, sc.part_e, n_e, v.et, v.att, v.att_w, v.src_off, g.att, g.embW, g.embb, part_a_ld()};
}
// the partial rows of the edge term's dL/d(att[:, mid block]) (a level whose edge term is a table of row dots): their column sums
int edge_term_colsum(ParamGradQueue& rq, const LevelView& v, const LevelWeights& g, const LevelScratch& sc, int n_rd) {
    return rq.colsum(sc.part_rd, n_rd, v.H * FN_D, g.att, v.att_w, v.mid_off, part_rd_ld(v.H));
}
// queued in the order finalize, [column sum], weight gradient (a lone partial product is launched on `launch_on`)
int level_params(ParamGradQueue& rq, const LevelView& v, const LevelWeights& g, const LevelScratch& sc, const ParamWork& o, hipStream_t launch_on) {
    FN_TRY(rq.finalize(att_param_grads(v, g, sc, o.n_a, o.n_e)));
    if (o.n_rd) FN_TRY(edge_term_colsum(rq, v, g, sc, o.n_rd));
    return rq.wgrad(fni::ProjWgrad{sc.g_h, v.x, v.K, v.rows, sc.wg_ws, v.n_real, g.W, g.bias}, launch_on);
}

// the source pass alone (fn_gat_bwd_src_f32)
int launch_gat_bwd_src(const GatBwdSrcArgs& A, int heads, hipStream_t st) {
    if (A.nblk == 0) return 0;
    FN_TRY(with_heads(heads, [&](auto H) { hipLaunchKernelGGL((k_gat_bwd_src<FN_CV(H), kBwdRows>), dim3(A.nblk), dim3(kBwdRows * 32), 0, st, A); }));
    return launch_status("fn_gat_bwd_src_f32");
}

// ... of an engine level, into its scratch (the partial rows in the engine's layout)
int engine_bwd_src(const LevelView& v, const LevelScratch& sc, const float* g_out, float* g_h, int* n_part_a, hipStream_t st) {
    GatBwdSrcArgs A;
    if (int rc = prep_gat_bwd_src(g_out, v.a.h, sc.pz, sc.g_s_dst, v.att, v.att_w, 0, v.src_off, v.pl, g_h, sc.part_a, n_part_a, v.H, &A)) return rc;
    A.part_ld = part_a_ld();
    return launch_gat_bwd_src(A, v.H, st);
}

// source pass of a two-pass level + backward of its edge term <feat[e], att[:, mid block]> as ONE launch (k_gat_bwd_src_rd); they
// share nothing but their input dz.  g_out / g_h: the level's gradient rows in and out; feat: the raw rows of the level that provides
// the edge features, g_feat their gradient rows (accumulate: they hold a gradient already).  *n_rd = blocks of the edge-term part (0:
// the level has no real edges).
int bwd_src_and_edge_term(const LevelView& v, const LevelScratch& sc, const float* g_out, float* g_h, const float* feat, float* g_feat,
                          bool accumulate, int* n_part_a, int* n_rd, hipStream_t st) {
    const int heads = v.H;
    GatBwdSrcArgs A;
    if (int rc = prep_gat_bwd_src(g_out, v.a.h, sc.pz, sc.g_s_dst, v.att, v.att_w, 0, v.src_off, v.pl, g_h, sc.part_a, n_part_a, heads, &A)) return rc;
    A.part_ld = part_a_ld();
    *n_rd = v.pl->m_real > 0 ? row_grid(v.pl->m_real, tune(FN_TUNE_RD_BLOCKS) > 0 ? tune(FN_TUNE_RD_BLOCKS) : kRowDotsBwdBlocks) : 0;
    if (*n_rd == 0) return launch_gat_bwd_src(A, heads, st);
    RowDotsBwdArgs T{sc.dz, feat, v.att, v.att_w, v.mid_off, heads, *v.pl, g_feat, sc.part_rd, accumulate ? (const float*)g_feat : nullptr, 1, *n_rd};
    T.part_ld = part_rd_ld(heads);
    if (A.nblk == 0) {
        hipLaunchKernelGGL(k_row_dots_sorted_bwd, dim3(T.nblk), dim3(kBlock), 0, st, T);
        return launch_status("edge-term backward");
    }
    FN_TRY(with_heads(heads, [&](auto H) { hipLaunchKernelGGL((k_gat_bwd_src_rd<FN_CV(H), kBwdRows>), dim3(A.nblk + T.nblk), dim3(kBlock), 0, st, A, T); }));
    return launch_status("source pass + edge-term backward");
}

// GEMM tiles + edge-term blocks as one launch (k_lin_rd_cu: the dots ride in the products' epilogue; either part may be empty)
static int launch_lin_rd(LinTasks& T, const RowDotsBwdArgs& R, hipStream_t st) {
    int blocks = 0, live = 0;
    bool aligned = true;
    for (int i = 0; i < T.n; ++i) {
        if (T.t[i].M <= 0) continue;
        LinTask t = T.t[i];
        if (((uintptr_t)t.X | (uintptr_t)t.Bt | (uintptr_t)t.Y | (uintptr_t)t.bias | (uintptr_t)t.mk.y) & 15) aligned = false;
        if (t.cu.c && !t.cu.out2) return fail(FN_EINVAL, "input-gradient products: a task's dots need out2 / sigma");
        t.first = blocks;
        t.nblk = lin_blocks((t.M + kLinRows - 1) / kLinRows, 1);
        blocks += t.nblk;
        T.t[live++] = t;
    }
    T.n = live;  T.K = FN_D;  T.total = blocks;  T.base = 0;
    if (!live) {
        if (R.nblk) {
            hipLaunchKernelGGL(k_row_dots_sorted_bwd, dim3(R.nblk), dim3(kBlock), 0, st, R);
            return launch_status("edge-term backward");
        }
        return 0;
    }
    if (!aligned) return fail(FN_EINVAL, "input-gradient products: operands must be 16-byte aligned");
    hipLaunchKernelGGL(k_lin_rd_cu, dim3(blocks + R.nblk), dim3(kBlock), kLinSideLds, st, T, R);
    return launch_status("input-gradient products (+ row dots) + edge-term backward");
}

int enc_check(const fn_encoder* e) {
    if (!e) return fail(FN_EINVAL, "fn_encoder: null descriptor");
    if (e->n_layers < 1 || e->n_layers > FN_MAX_LAYERS) return fail(FN_EINVAL, "fn_encoder: n_layers out of range");
    if (e->heads != 1 && e->heads != 2 && e->heads != 4 && e->heads != 8) return fail(FN_EUNSUPPORTED, "fn_encoder: heads must be 1, 2, 4 or 8");
    if (e->variant < 0 || e->variant > 2) return fail(FN_EUNSUPPORTED, "fn_encoder: variant must be 0 (gat2), 1 (gat2_lite) or 2 (gat2_edge)");
    if (e->k_atom0 < 1 || e->k_atom0 > 168 || e->k_bond0 < 1 || e->k_bond0 > 168 || e->k_fbond0 < 1 || e->k_fbond0 > 168)
        return fail(FN_EUNSUPPORTED, "fn_encoder: layer-0 feature widths must be in [1, 168]");
    if (e->k_fattr < 1 || e->k_fattr > FN_MAX_EDGE_K) return fail(FN_EUNSUPPORTED, "fn_encoder: fragment-bond attribute width");
    if (e->bond.n != e->E || e->atom.n != e->N || e->fbond.n != e->EF || e->frag.n != e->F || e->a2f.n_seg != e->F || e->a2f.n_items != e->N)
        return fail(FN_EINVAL, "fn_encoder: plan sizes disagree with N/E/F/EF");
    if (e->atom.m_real != e->E || e->frag.m_real != e->EF) return fail(FN_EINVAL, "fn_encoder: bond nodes must be the atom-graph edges");
    if (!e->x_atoms || !e->bond_nodes || !e->fbond_nodes || !e->cos_sorted || !e->fattr_sorted || !e->ws)
        return fail(FN_EINVAL, "fn_encoder: null input");
    return 0;
}

int launch_tail_fwd(const fn_encoder* e, const EncLayout& lay, const LevelView& vf, const fn_act_epilogue& ep_frags, const float* y_atoms,
                    hipStream_t st) {
    const int H = e->heads;
    TailFwdArgs T{};
    T.ext = reinterpret_cast<const MolExt*>(lay.mol_ext);  T.n_mols = (int)e->n_mols;  T.counts_dev = e->counts_dev;
    T.atoms_new = lay.atoms_new;  T.a2f_rowptr = e->a2f.rowptr;  T.a2f_perm = e->a2f.perm;  T.a2f_base = e->a2f.pos_base;  T.a2f_items = (int)e->a2f.n_items;
    T.frags = vf.a.h;  T.att = vf.att;  T.att_w = vf.att_w;  T.dst_off = 0;  T.src_off = vf.src_off;  T.mid_off = vf.mid_off;
    T.s_dst = vf.s_dst;  T.s_src = vf.s_src;  T.feat = lay.L[vf.layer].lv[LV_FBOND].raw;  T.s_sorted = lay.s_sorted;
    const fn_edge_term et_f = fwd_edge_term(vf, lay.s_sorted);
    FN_TRY(prep_gat_fwd(vf.a.h, vf.s_dst, vf.s_src, vf.att, vf.att_w, &et_f, vf.pl, 0.2f, nullptr, vf.a.p, nullptr, &ep_frags, H, &T.G));
    T.y_atoms = y_atoms;  T.pooled = e->pooled;  T.force_global = tune(FN_TUNE_MOL_TAIL) == 2;
    if (((uintptr_t)y_atoms | (uintptr_t)ep_frags.y | (uintptr_t)e->pooled) & 15) return fail(FN_EINVAL, "fragment tail: outputs must be 16-byte aligned");
    const dim3 grid((unsigned)e->n_mols);
    with_const<2, 4, 8>(H, [&](auto h) { hipLaunchKernelGGL((k_tail_fwd<FN_CV(h)>), grid, dim3(kBlock), 0, st, T); });      // (tail_mol_on: one of them)
    return launch_status("fragment tail, molecule-resident (sums + fragment graph + readout)");
}

// y / gy: the forward's outputs and the gradients w.r.t. them (atoms and fragments are read).  Partial rows written: one per
// molecule (*n_part), for rq.finalize (part_a) and rq.colsum (part_rd)
// one_pass_dots: the last layer's atom and fragment-bond levels run the one-pass backward next: their rows' dots from here
int launch_tail_bwd(const fn_encoder* e, const EncLayout& lay, const BwdLayout& bw, const EncOutputs& y, const EncOutputs& gy, bool accumulate_fbond,
                    int* n_part, hipStream_t st, bool one_pass_dots = false, bool* rider_done = nullptr) {
    const int H = e->heads, l = e->n_layers - 1;
    const LevelView vf = level_view(e, lay, l, LV_FRAG), va = level_view(e, lay, l, LV_ATOM), vfb = level_view(e, lay, l, LV_FBOND);
    const LevelScratch& sf = bw.frag;
    const float *y_atoms = y.y[LV_ATOM], *y_frags = y.y[LV_FRAG], *g_atoms = gy.y[LV_ATOM], *g_frags = gy.y[LV_FRAG];
    TailBwdArgs T{};
    T.ext = reinterpret_cast<const MolExt*>(lay.mol_ext);  T.n_mols = (int)e->n_mols;  T.counts_dev = e->counts_dev;
    T.g_atoms = g_atoms;  T.g_frags = g_frags;  T.g_pooled = e->g_pooled;  T.y_atoms = y_atoms;  T.y_frags = y_frags;  T.scale = gate_scale(e);
    T.g_pre_atoms = bw.g_pre[LV_ATOM];  T.g_pre_frags = bw.g_pre[LV_FRAG];  T.a2f_index = e->a2f.index;  T.n_atoms = e->N;  T.force_global = tune(FN_TUNE_MOL_TAIL) == 2;
    int n_e = 0, n_a = 0;
    FN_TRY(prep_gat_bwd_dst(bw.g_pre[LV_FRAG], vf.a.h, vf.a.p, &vf.et, vf.pl, 0.2f, nullptr, sf.dz, sf.pz, sf.g_s_dst, nullptr, &n_e, H, &T.D));
    FN_TRY(prep_gat_bwd_src(bw.g_pre[LV_FRAG], vf.a.h, sf.pz, sf.g_s_dst, vf.att, vf.att_w, 0, vf.src_off, vf.pl, bw.g_frags, sf.part_a, &n_a, H, &T.S));
    T.R = RowDotsBwdArgs{sf.dz, vfb.a.raw, vf.att, vf.att_w, vf.mid_off, H, *vf.pl, bw.g_pre[LV_FBOND], sf.part_rd,
                         accumulate_fbond ? (const float*)bw.g_pre[LV_FBOND] : (const float*)nullptr, 1, 0};
    T.S.part_ld = part_a_ld();  T.R.part_ld = part_rd_ld(H);
    if (one_pass_dots) {
        const LevelScratch &sa = bw.lv[l][LV_ATOM], &sfb = bw.lv[l][LV_FBOND];
        T.cu_out = va.a.raw;  T.cu_out2 = va.a.o2;  T.cu_sigma = va.a.sg;  T.cu_c = sa.cdot;  T.cu_u = sa.g_s_dst;
        if (H == 4) { T.R.cu_out2 = vfb.a.o2;  T.R.cu_sigma = vfb.a.sg;  T.R.cu_c = sfb.cdot;  T.R.cu_u = sfb.g_s_dst; }
    }
    if (((uintptr_t)y_atoms | (uintptr_t)y_frags | (uintptr_t)g_atoms | (uintptr_t)g_frags | (uintptr_t)e->g_pooled) & 15)
        return fail(FN_EINVAL, "fragment tail backward: gradients must be 16-byte aligned");
    // the first launch of the backward pass is latency-bound (one workgroup per molecule, 2 of 3 slots per CU taken): the head's Adam
    // slice (fn_encoder.adam_rider) can stream beside it (FN_TUNE_RIDER_AT = 1; measured: this launch 18.5 -> 30.2 us, against
    // 15.4 -> 22.5 us for the deferred-reduction launch, the default); *rider_done tells the caller
    AdamRide R{};
    if (rider_done) {
        *rider_done = false;
        if (tune(FN_TUNE_RIDER_AT) == 1 && e->adam_rider) {
            R = make_adam_ride(e->adam_rider, (int)e->n_mols, kBlock, tune(FN_TUNE_RIDER_PIECES));
            *rider_done = R.nblk > 0;
        }
    }
    const dim3 grid((unsigned)(e->n_mols + R.nblk));
    with_const<2, 4, 8>(H, [&](auto h) { hipLaunchKernelGGL((k_tail_bwd<FN_CV(h)>), grid, dim3(kBlock), 0, st, T, R); });
    *n_part = (int)e->n_mols;
    const int rc = launch_status("fragment tail backward, molecule-resident (gates + fragment graph + scatter to atoms)");
    if (rc == 0 && R.nblk > 0) e->adam_rider->launched = 1;
    return rc;
}

// ---- the last layer's output gradients, for both backward forms: the gates of relu(dropout(.)) of the four outputs (one launch; y > 0
// already encodes the mask), the fragment graph -- the only layer whose fragment level is ever read -- and the scatter of
// dL/d(fragment sums) back to the atoms.  Leaves the pre-activation gradients of the last layer's three projected levels in bw.g_pre.
struct LastGrads {
    bool have[kLevels];                          // by Level: g_pre holds the level's gradient rows (else: zero, not written)
    bool tail_dots_atoms, tail_dots_fbond;       // one-pass form: the fragment tail's launch wrote the level's dots as well
};
// one_pass: the caller runs the one-pass backward next -- the molecule-resident tail writes the dots of the rows it finishes and may
// carry the Adam rider (which then leaves rq)
int last_layer_output_grads(const fn_encoder* e, const EncLayout& lay, const BwdLayout& bw, const EncOutputs& y, const EncOutputs& gy,
                            const fn_layer_weights* grads, ParamGradQueue& rq, bool one_pass, hipStream_t hs, LastGrads* out) {
    const int H = e->heads, l = e->n_layers - 1;
    const bool lite = e->variant == 1, edge = e->variant == 2;
    const LevelView vf = level_view(e, lay, l, LV_FRAG);
    const LevelWeights gf = level_weights(grads[l], LV_FRAG, e->variant);
    const LevelScratch& sf = bw.frag;
    // molecule-resident tail (csrc/mol_tail.inc): the atoms' and fragments' gates, the fragment graph's two passes, its edge term's
    // backward and the scatter to the atoms are ONE launch below; the readout's gradient enters there
    const bool tail_mol = tail_mol_on(e) && (gy.y[LV_FRAG] != nullptr || e->g_pooled != nullptr);
    bool have_atoms = gy.y[LV_ATOM] != nullptr, have_fbond = gy.y[LV_FBOND] != nullptr;
    const bool have_frags = gy.y[LV_FRAG] != nullptr;
    GateTasks G{};
    auto add = [&](Level v) {
        if (!gy.y[v]) return;
        GateTask& t = G.t[G.n++];
        t.g = gy.y[v];  t.y = y.y[v];  t.o = bw.g_pre[v];  t.n4 = (level_rows(e, v) * FN_D + 3) / 4;  t.first = G.blocks;  t.nblk = flat_grid(t.n4, 512);
        G.blocks += t.nblk;
    };
    if (!tail_mol) { add(LV_ATOM);  add(LV_FRAG); }
    add(LV_BOND);
    add(LV_FBOND);
    if (G.blocks) {
        G.scale = gate_scale(e);
        hipLaunchKernelGGL(k_gate_many, dim3(G.blocks), dim3(kBlock), 0, hs, G);
        FN_TRY(launch_status("fn_encoder_backward: activation backward"));
    }
    bool have_g_frags_h = false;
    const float* g_frags_h = bw.g_frags;      // dL/d(fragment sums), scattered back to the atoms below
    int n_a = 0, n_e = 0;
    if (tail_mol) {
        int n_part = 0;
        bool rode = false;
        FN_TRY(launch_tail_bwd(e, lay, bw, y, gy, have_fbond, &n_part, hs, one_pass, one_pass ? &rode : nullptr));
        if (rode) rq.rider = nullptr;          // the head's Adam slice went with this launch
        FN_TRY(rq.finalize(att_param_grads(vf, gf, sf, n_part, 0)));
        FN_TRY(edge_term_colsum(rq, vf, gf, sf, n_part));
        have_atoms = have_fbond = true;        // g_pre of the atoms and fragment bonds is complete (scatter to the atoms included)
        out->tail_dots_atoms = one_pass;  out->tail_dots_fbond = one_pass && H == 4;
    } else if (have_frags && lite) {
        g_frags_h = bw.g_pre[LV_FRAG];         // no fragment graph in between
        have_g_frags_h = true;
    } else if (have_frags && edge) {   // gat2_edge: the edge term's parameters are the cnx_attr Linear (emb_fb_*) and f's middle block
        FN_TRY(fn_gat_bwd_dst_f32(bw.g_pre[LV_FRAG], vf.a.h, vf.a.p, &vf.et, vf.pl, 0.2f, nullptr, nullptr, sf.pz, sf.g_s_dst, sf.part_e, &n_e, H, hs));
        FN_TRY(engine_bwd_src(vf, sf, bw.g_pre[LV_FRAG], bw.g_frags, &n_a, hs));
        FN_TRY(rq.finalize(att_param_grads(vf, gf, sf, n_a, n_e)));
        have_g_frags_h = true;
    } else if (have_frags) {
        FN_TRY(fn_gat_bwd_dst_f32(bw.g_pre[LV_FRAG], vf.a.h, vf.a.p, &vf.et, vf.pl, 0.2f, nullptr, sf.dz, sf.pz, sf.g_s_dst, nullptr, &n_e, H, hs));
        // source pass + edge term <new_fbond, f[:, d:d+128]> (dL/dnew_fbond accumulates into g_pre of the fragment bonds, dL/df mid block)
        int gr = 0;
        FN_TRY(bwd_src_and_edge_term(vf, sf, bw.g_pre[LV_FRAG], bw.g_frags, lay.L[l].lv[LV_FBOND].raw, bw.g_pre[LV_FBOND], have_fbond, &n_a, &gr, hs));
        if (gr) have_fbond = true;
        FN_TRY(rq.finalize(att_param_grads(vf, gf, sf, n_a, 0)));
        if (gr) FN_TRY(edge_term_colsum(rq, vf, gf, sf, gr));
        have_g_frags_h = true;
    }
    // atom -> fragment sum: dL/datoms_new += dL/dfrags[a2f]
    if (have_g_frags_h) {
        FN_TRY(launch_gather_rows4(g_frags_h, e->a2f.index, bw.g_pre[LV_ATOM], e->N, 32, have_atoms ? (const float*)bw.g_pre[LV_ATOM] : (const float*)nullptr, hs,
                                   "fn_encoder_backward: gather(a2f)"));
        have_atoms = true;
    }
    out->have[LV_ATOM] = have_atoms;  out->have[LV_BOND] = gy.y[LV_BOND] != nullptr;  out->have[LV_FBOND] = have_fbond;
    return 0;
}

// ---- fn_encoder_backward with every attention level as ONE source-owner pass (csrc/gat_bwd_one.inc, FN_TUNE_BWD_ONE).
// Gradient flows atom level -> bond levels only (through the edge term <new_bond[e], a[:, mid]>), so the atom level of layer l and
// the bond / fragment-bond levels of layer l+1 are ready together: two launches per layer,
//   L1  k_gat_bwd_one3 { bond level (l+1), atom level (l), fragment-bond level (l+1) }
//   L2  k_lin_rd_cu    { dX of the atom projection (l) -> dL/d(atom rows of layer l-1); dX of the bond projection (l+1) + the atom
//                        graph's edge-term gradient of layer l on the rows it writes (RowAdd) -> dL/d(bond rows of layer l); dX of
//                        the fragment-bond projection (l+1) }  ||  the edge term's parameter partials,
// and the products' epilogue (CuEpi) leaves the two node-local dots c = <g, out>, g_s_dst = <g, out2> - c sigma of every row it
// finishes, which is all the next L1 needs besides the rows themselves.  Rows whose gradient is completed elsewhere (the last
// layer's: by the fragment tail / the gates / the edge-term backward) get their dots from k_gat_cu.  Weight-gradient partial
// products and parameter reductions are queued for the two launches at the very end, as in the two-pass path.
int encoder_backward_one(const fn_encoder* e, const EncLayout& lay, const BwdLayout& bw, const RngPlan& rng, const EncOutputs& y,
                         const EncOutputs& gy, const fn_layer_weights* grads, hipStream_t hs) {
    const int H = e->heads, NL = e->n_layers;
    const bool no_fb = e->variant != 0;          // gat2_lite / gat2_edge: neither has a fragment-bond graph
    ParamGradQueue rq;
    rq.st = hs;
    rq.defer_mixed = tune(FN_TUNE_GEMM_COLAUNCH) != 0;
    rq.rider = e->adam_rider;
    struct Parts { int n_a = 0, n_e = 0; };      // partial rows a level's pass wrote (attention vector / edge embedding)
    // a level's pass, prepared for the launch that carries it.  (Sharing a fixed total of workgroups out among the levels of a launch by
    // their items -- fewer, longer-lived workgroups -- measured 40-50 us against 33 for the launch of layer l: every level sizes itself)
    auto one_level = [&](const LevelView& v, const LevelScratch& sc, Parts* n, GatBwdOneArgs* A) -> int {
        // (sc.dz: the atom level's dL/d(edge term) in original edge order; the other levels have none)
        FN_TRY(prep_gat_bwd_one(bw.g_pre[v.lv], v.a.h, v.a.p, sc.cdot, sc.g_s_dst, &v.et, v.att, v.att_w, 0, v.src_off, v.pl, 0.2f, sc.g_h, nullptr, sc.dz,
                                sc.part_a, &n->n_a, sc.part_e, &n->n_e, H, A));
        A->p_edge_major = 1;
        A->n_real = v.n_real;
        A->part_ld = part_a_ld();
        return 0;
    };
    auto scratch = [&](const LevelView& v) -> const LevelScratch& { return bw.lv[v.layer][v.lv]; };
    // rows of level v whose gradient is complete but whose dots no epilogue wrote: a task of k_gat_cu
    auto cu_add = [&](CuTasks& T, const LevelView& v) {
        const LevelScratch& sc = scratch(v);
        if (v.rows > 0) T.t[T.n++] = CuTask{bw.g_pre[v.lv], v.a.raw, v.a.o2, v.a.sg, 1.f, sc.cdot, sc.g_s_dst, v.rows, 0, 0};
    };
    // ... or the epilogue of the product that finishes them (raw: the product's rows are gradients of the raw rows; else of y, whose
    // saved copy stands in -- an inner layer's atom and fragment-bond rows get gradient through relu(dropout(.)) only)
    auto cu_epi = [&](const LevelView& v, bool raw, bool dots = true) {
        const LevelScratch& sc = scratch(v);
        return CuEpi{raw ? v.a.raw : nullptr, v.a.o2, v.a.sg, dots ? sc.cdot : nullptr, sc.g_s_dst, H};
    };

    // ---- the last layer's output gradients: gates, the fragment levels, the scatter to the atoms
    LastGrads top{};
    FN_TRY(last_layer_output_grads(e, lay, bw, y, gy, grads, rq, true, hs, &top));
    // g_pre of the CURRENT layer complete, dots written
    bool have_atoms = top.have[LV_ATOM], have_bond = top.have[LV_BOND], have_fbond = top.have[LV_FBOND] && !no_fb;
    CuTasks cu_now{};         // rows of the current layer whose dots no product epilogue wrote
    if (have_atoms && !top.tail_dots_atoms) cu_add(cu_now, level_view(e, lay, NL - 1, LV_ATOM));

    bool pend_b = false, pend_fb = false;        // bond / fragment-bond level of layer l+1: gradient rows and dots ready, pass not launched
    for (int l = NL - 1; l >= 0; --l) {
        const bool last = l + 1 == NL;
        // this layer's levels (the atom level runs now; the other two receive their gradient rows), the atom level below, and the bond /
        // fragment-bond levels of layer l+1, which run now
        const LevelView va = level_view(e, lay, l, LV_ATOM), vb = level_view(e, lay, l, LV_BOND), vfb = level_view(e, lay, l, LV_FBOND);
        const LevelView va_below = l ? level_view(e, lay, l - 1, LV_ATOM) : LevelView{};
        const LevelView vb_up = last ? LevelView{} : level_view(e, lay, l + 1, LV_BOND), vfb_up = last ? LevelView{} : level_view(e, lay, l + 1, LV_FBOND);
        const LevelWeights ga = level_weights(grads[l], LV_ATOM);
        const LevelScratch& sa = bw.lv[l][LV_ATOM];
        if (cu_now.n) { FN_TRY(launch_gat_cu(cu_now, H, hs));  cu_now = CuTasks{}; }

        // ---- L1: the atom level of this layer beside the bond / fragment-bond levels of layer l+1
        GatBwdOneArgs oB{}, oA{}, oFB{};
        Parts nb, na, nfb;
        if (pend_b) FN_TRY(one_level(vb_up, scratch(vb_up), &nb, &oB));
        if (have_atoms) FN_TRY(one_level(va, sa, &na, &oA));
        if (pend_fb) FN_TRY(one_level(vfb_up, scratch(vfb_up), &nfb, &oFB));
        FN_TRY(launch_gat_bwd_one3(oB, oA, oFB, H, hs));

        // ---- L2: input-gradient products of what L1 produced (+ the atom graph's edge term), and the deferred parameter work
        LinTasks T{};
        CuTasks cu_after{};       // rows finished in L2 whose dots the epilogue could not write
        // dX of level v's projection: the gradient rows of the same level one layer down (`below`), gated by that layer's dropout mask and ReLU
        auto product = [&](const LevelView& v, const LevelView& below, const RowAdd* ra, const CuEpi& cu) {
            LinTask& t = T.t[T.n++];
            t = LinTask{v.Wt, scratch(v).g_h, v.W, nullptr, bw.g_pre[v.lv], v.rows, act_epilogue(e, rng, below, below.a.y),
                        NodeScalarEpi{nullptr, nullptr, nullptr, 0, 0, 0, 0}, 0, 0};
            if (ra) t.ra = *ra;
            t.cu = cu;
            t.n_real = v.n_real;
        };
        bool nxt_bond = false, nxt_fbond = false, nxt_atoms = false;
        const bool rd_rows_ride = have_atoms && pend_b && H == 4 && e->atom.m_real == e->E && e->E > 0;   // the bond product of layer l+1 carries the rows' term
        const int gr = have_atoms && e->atom.m_real > 0 ? row_grid(e->atom.m_real, tune(FN_TUNE_RD_BLOCKS) > 0 ? tune(FN_TUNE_RD_BLOCKS) : kRowDotsBwdBlocks) : 0;
        if (pend_b) {        // layer l+1's bond level: parameter work + dL/d(pre-activation bond output of layer l)
            FN_TRY(level_params(rq, vb_up, level_weights(grads[l + 1], LV_BOND), scratch(vb_up), ParamWork{nb.n_a, nb.n_e}, hs));
            const RowAdd ra{sa.dz, va.att + va.mid_off, va.att_w};
            // the rows are complete in this epilogue unless the edge term's rows' part is added behind the product (no RowAdd carrier)
            const bool complete = rd_rows_ride || gr == 0;
            product(vb_up, vb, rd_rows_ride ? &ra : nullptr, cu_epi(vb, true, complete));
            if (!complete) cu_add(cu_after, vb);
            nxt_bond = true;
        }
        if (pend_fb) {
            FN_TRY(level_params(rq, vfb_up, level_weights(grads[l + 1], LV_FBOND), scratch(vfb_up), ParamWork{nfb.n_a, nfb.n_e}, hs));
            // (the fragment graph's edge term, the only reader of raw fragment-bond rows, exists in the last layer alone)
            product(vfb_up, vfb, nullptr, cu_epi(vfb, false));
            nxt_fbond = true;
        }
        RowDotsBwdArgs R{};
        if (have_atoms) {
            FN_TRY(level_params(rq, va, ga, sa, ParamWork{na.n_a, 0}, hs));
            if (l) {
                product(va, va_below, nullptr, cu_epi(va_below, false));
                nxt_atoms = true;
            }
            // the edge term <new_bond[e], a[:, d:d+128]> of the atom graph: parameter partials always; the rows' term (dL/dnew_bond)
            // rides in the bond product above, or -- no product to ride in (top layer, H != 4) -- is written / accumulated here
            if (gr) {
                const bool have_b_now = pend_b || (last && have_bond);
                R = RowDotsBwdArgs{sa.dz, vb.a.raw, va.att, va.att_w, va.mid_off, H, *va.pl, rd_rows_ride ? nullptr : bw.g_pre[LV_BOND], sa.part_rd,
                                   (!rd_rows_ride && have_b_now) ? (const float*)bw.g_pre[LV_BOND] : nullptr, 1, gr};
                R.n_real = vb.n_real;
                R.part_ld = part_rd_ld(H);
                FN_TRY(edge_term_colsum(rq, va, ga, sa, gr));
                if (!pend_b) {
                    // the bond rows of this layer are finished by the edge term's rows' part: with four heads it writes their dots too
                    const LevelScratch& sb = scratch(vb);
                    if (H == 4 && e->atom.m_real == e->E) { R.cu_out2 = vb.a.o2;  R.cu_sigma = vb.a.sg;  R.cu_c = sb.cdot;  R.cu_u = sb.g_s_dst; }
                    else cu_add(cu_after, vb);
                }
                nxt_bond = true;
            }
        }
        if (R.nblk && !rd_rows_ride && pend_b) {
            // (no RowAdd carrier: the product first, the rows' term accumulates behind it)
            FN_TRY(launch_lin_rd(T, RowDotsBwdArgs{}, hs));
            T = LinTasks{};
        }
        FN_TRY(launch_lin_rd(T, R, hs));

        // ---- what the next iteration's L1 finds
        if (last) {
            if (have_bond && !nxt_bond) cu_add(cu_after, vb);
            if (have_fbond && !top.tail_dots_fbond) cu_add(cu_after, vfb);
            nxt_bond = nxt_bond || have_bond;
            nxt_fbond = nxt_fbond || have_fbond;
        }
        pend_b = nxt_bond;
        pend_fb = nxt_fbond && !no_fb;
        have_atoms = nxt_atoms;
        have_bond = have_fbond = false;
        cu_now = cu_after;
    }
    {   // the bond / fragment-bond levels of layer 0
        if (cu_now.n) FN_TRY(launch_gat_cu(cu_now, H, hs));
        const LevelView vb = level_view(e, lay, 0, LV_BOND), vfb = level_view(e, lay, 0, LV_FBOND);
        const LevelScratch &sb = scratch(vb), &sfb = scratch(vfb);
        GatBwdOneArgs oB{}, oFB{};
        Parts nb, nfb;
        if (pend_b) FN_TRY(one_level(vb, sb, &nb, &oB));
        if (pend_fb) FN_TRY(one_level(vfb, sfb, &nfb, &oFB));
        FN_TRY(prof_event(2, hs));
        FN_TRY(launch_gat_bwd_one3(oB, GatBwdOneArgs{}, oFB, H, hs));
        FN_TRY(prof_event(3, hs));
        if (pend_b) FN_TRY(level_params(rq, vb, level_weights(grads[0], LV_BOND), sb, ParamWork{nb.n_a, nb.n_e}, hs));
        if (pend_fb) FN_TRY(level_params(rq, vfb, level_weights(grads[0], LV_FBOND), sfb, ParamWork{nfb.n_a, nfb.n_e}, hs));
    }
    return rq.flush(true);
}


}  // namespace

// forward declaration: the pass behind fn_encoder_forward and fn_encoder_forward_masked (defined with them, below)
static int encoder_forward_impl(const fn_encoder* e, const fn_row_masks* masks, const fn_attn_readout* readout, float* out_atoms,
                                float* out_frags, float* out_bond, float* out_fbond, fn_stream_t st, const uint8_t* keep_atoms = nullptr);

extern "C" {

int fn_encoder_fused_tail(const fn_encoder* e) { return e && tail_mol_on(e) ? 1 : 0; }

int64_t fn_encoder_ws_floats(const fn_encoder* e) { return e ? enc_layout(e, nullptr).total : 0; }
int64_t fn_encoder_keep_ws_floats(const fn_encoder* e) { return e ? enc_layout(e, nullptr, true).total : 0; }
int64_t fn_encoder_bwd_ws_floats(const fn_encoder* e) { return e ? bwd_layout(e, nullptr).total : 0; }
uint64_t fn_encoder_rng_blocks(const fn_encoder* e) { return e ? rng_plan(e).total : 0; }

int fn_encoder_forward(const fn_encoder* e, float* out_atoms, float* out_frags, float* out_bond, float* out_fbond,
                       fn_stream_t st) {
    return encoder_forward_impl(e, nullptr, nullptr, out_atoms, out_frags, out_bond, out_fbond, st);
}

int fn_encoder_forward_masked(const fn_encoder* e, const fn_row_masks* m, float* out_atoms, float* out_frags, float* out_bond,
                              float* out_fbond, fn_stream_t st) {
    if (!m || (!m->atoms && !m->bonds && !m->fbonds)) return encoder_forward_impl(e, nullptr, nullptr, out_atoms, out_frags, out_bond, out_fbond, st);
    // everything a masked pass can be refused for is decided here, before the first launch
    FN_TRY(enc_check(e));
    if (e->variant != 0) return fail(FN_EUNSUPPORTED, "fn_encoder_forward_masked: row masks exist for variant 0 (gat2); gat2_lite / gat2_edge have no masks in the reference");
    if (e->training != 0) return fail(FN_EINVAL, "fn_encoder_forward_masked: a masked pass is an evaluation pass (training must be 0)");
    if (e->no_backward == 0) return fail(FN_EINVAL, "fn_encoder_forward_masked: a masked pass has no backward (no_backward must be 1)");
    if (e->heads != 4) return fail(FN_EUNSUPPORTED, "fn_encoder_forward_masked: the masked attention instances are built for four heads");
    return encoder_forward_impl(e, m, nullptr, out_atoms, out_frags, out_bond, out_fbond, st);
}

int fn_encoder_forward_keep(const fn_encoder* e, const uint8_t* keep_atoms, float* out_atoms, float* out_frags, float* out_bond,
                            float* out_fbond, fn_stream_t st) {
    if (!keep_atoms) return encoder_forward_impl(e, nullptr, nullptr, out_atoms, out_frags, out_bond, out_fbond, st);
    // everything a gated pass can be refused for is decided here, before the first launch
    FN_TRY(enc_check(e));
    if (e->variant != 0) return fail(FN_EUNSUPPORTED, "fn_encoder_forward_keep: the input gate exists for variant 0 (gat2): the reference masks atoms in FragNetPreTrainMasked2 only");
    return encoder_forward_impl(e, nullptr, nullptr, out_atoms, out_frags, out_bond, out_fbond, st, keep_atoms);
}

int fn_encoder_forward_attn(const fn_encoder* e, const fn_attn_readout* r, float* out_atoms, float* out_frags, float* out_bond,
                            float* out_fbond, fn_stream_t st) {
    if (!r || (!r->atoms && !r->frags && !r->bonds && !r->fbonds)) return encoder_forward_impl(e, nullptr, nullptr, out_atoms, out_frags, out_bond, out_fbond, st);
    // everything a read-out pass can be refused for is decided here, before the first launch
    FN_TRY(enc_check(e));
    if (e->variant != 0) return fail(FN_EUNSUPPORTED, "fn_encoder_forward_attn: the attention read-out exists for variant 0 (gat2); the reference's gat2_lite / gat2_edge Viz classes cannot run");
    if (e->training != 0) return fail(FN_EINVAL, "fn_encoder_forward_attn: a read-out pass is an evaluation pass (training must be 0)");
    return encoder_forward_impl(e, nullptr, r, out_atoms, out_frags, out_bond, out_fbond, st);
}

}  // extern "C" (reopened behind the pass itself)

// masks == null: the plain pass.  Else the caller has checked that the descriptor is one a masked pass exists for, and every attention
// level of the three masked index spaces launches forward kind 4 (gat_fwd.inc) with its byte array (null inside: no masked row there).
// The fragment graph has no mask (gat2.py has none), and everything behind the three levels reads stored rows.
// readout != null (never together with masks; the caller has checked variant 0 and an evaluation pass): the last layer's levels store
// their probabilities whatever no_backward says, and ONE more launch behind the last level sums them by source (attn_readout.hip).
// keep_atoms != null (never together with masks or a read-out; the caller has checked variant 0): the input gate of x_atoms, folded into
// the prologue's dropout block range; everything behind it reads the gated (and dropped) copy through the atom level's view.
static int encoder_forward_impl(const fn_encoder* e, const fn_row_masks* masks, const fn_attn_readout* readout, float* out_atoms,
                                float* out_frags, float* out_bond, float* out_fbond, fn_stream_t st, const uint8_t* keep_atoms) {
    FN_TRY(enc_check(e));
    if (!out_atoms || !out_frags) return fail(FN_EINVAL, "fn_encoder_forward: null output");
    if ((out_bond == nullptr) != (out_fbond == nullptr)) return fail(FN_EINVAL, "fn_encoder_forward: out_bond and out_fbond are wanted together or not at all");
    if (e->pooled && !tail_mol_on(e)) return fail(FN_EINVAL, "fn_encoder_forward: the readout is only produced by the fused fragment tail (fn_encoder_fused_tail)");
    const EncLayout lay = enc_layout(e, e->ws, keep_atoms != nullptr);
    if (lay.total > e->ws_floats) return fail(FN_EINVAL, "fn_encoder_forward: workspace too small");
    latch_form(e, keep_atoms != nullptr);
    const RngPlan rng = rng_plan(e);
    const int H = e->heads;
    const float p = e->training ? e->drop_p : 0.f;
    const bool lite = e->variant == 1, edge = e->variant == 2;      // gat2_lite / gat2_edge: neither has a fragment-bond graph
    const bool no_fb = lite || edge;
    // the atom graph's edge term <new_bond, a[:, d:d+128]> is produced by the bond-graph kernel's epilogue (one launch less per layer)
    const bool fuse_rd = tune(FN_TUNE_FUSE_ROWDOTS) != 0 && e->atom.m > 0 && e->atom.m_real == e->E;
    // projections ride along with the attention launches they do not depend on (k_gat_*_lin); needs the node scalars in the GEMM epilogue
    const bool colaunch = H >= 2 && tune(FN_TUNE_GEMM_COLAUNCH) != 0;
    // the backward will be one source-owner pass per level: the attention kernels also write out2 / sigma, probabilities edge-major
    const bool one = one_pass_on(e);
    // an evaluation pass that nobody differentiates (fn_encoder.no_backward) saves nothing for a backward pass: no probabilities, and no
    // raw bond rows once the atom graph's edge term is formed in the bond level's own launch
    const bool no_bwd = !e->training && e->no_backward != 0;
    const fni::FwdMask mk_atoms{masks ? masks->atoms : nullptr}, mk_bonds{masks ? masks->bonds : nullptr}, mk_fbonds{masks ? masks->fbonds : nullptr};
    const fni::FwdMask *pm_atoms = masks ? &mk_atoms : nullptr, *pm_bonds = masks ? &mk_bonds : nullptr, *pm_fbonds = masks ? &mk_fbonds : nullptr;

    {   // one launch: W^T of every projection, dropout(x_atoms), destination-order edge attributes
        EncPrologue A{};
        for (int l = 0; l < e->n_layers; ++l)
            for (Level v : kProjected) {
                const LevelView lv = level_view(e, lay, l, v);
                A.tm.W[3 * l + v] = lv.W;  A.tm.K[3 * l + v] = lv.K;
                if (!lv.W) return fail(FN_EINVAL, "fn_encoder_forward: null projection weight");
            }
        A.bt_base = lay.bt;
        A.n_t = 24 * 3 * e->n_layers;
        if (lay.in_atoms0) {
            A.dx = e->x_atoms;  A.dy = lay.in_atoms0;  A.dnumel = e->N * e->k_atom0;  A.p = p;  A.seed = e->seed;
            A.offset = rng.in_atoms;  A.offset_dev = e->offset_dev;
            A.dgate = keep_atoms;  A.dgate_w = e->k_atom0;
            A.n_d = flat_grid((A.dnumel + 3) / 4, 512);
        }
        if (e->cos_raw && e->bond.m > 0) {
            A.sx[0] = e->cos_raw;  A.so[0] = const_cast<float*>(e->cos_sorted);  A.sK[0] = 1;  A.spl[0] = e->bond;
            A.n_s[0] = flat_grid(e->bond.m, 512);
        }
        const fn_gat_plan& fattr_plan = edge ? e->frag : e->fbond;     // gat2_edge: cnx_attr rides on the fragment graph's edges
        if (e->fattr_raw && fattr_plan.m > 0) {
            A.sx[1] = e->fattr_raw;  A.so[1] = const_cast<float*>(e->fattr_sorted);  A.sK[1] = e->k_fattr;  A.spl[1] = fattr_plan;
            A.n_s[1] = flat_grid(fattr_plan.m * e->k_fattr, 512);
        }
        if (one) {
            if (e->bond.m > 0) {
                A.ssr[0] = e->cos_raw;  A.sss[0] = e->cos_sorted;  A.sso[0] = lay.xs_bond;  A.sK[0] = 1;  A.spl[0] = e->bond;
                A.n_ss[0] = flat_grid(e->bond.m, 512);
            }
            if (!no_fb && e->fbond.m > 0) {
                A.ssr[1] = e->fattr_raw;  A.sss[1] = e->fattr_sorted;  A.sso[1] = lay.xs_fbond;  A.sK[1] = e->k_fattr;  A.spl[1] = e->fbond;
                A.n_ss[1] = flat_grid(e->fbond.m * e->k_fattr, 512);
            }
        }
        if (tail_mol_on(e) || pad_skip_on(e)) {
            A.mx = MolExtArgs{e->mol_atoms.rowptr, e->mol_frags.rowptr, e->mol_atoms.pos_base, e->mol_frags.pos_base,
                              e->bond, e->atom, no_fb ? fn_gat_plan{} : e->fbond, e->frag, (int)e->n_mols,
                              reinterpret_cast<MolExt*>(lay.mol_ext), e->counts_dev, reinterpret_cast<int32_t*>(lay.real_rows)};
            A.n_x = (int)((e->n_mols + 255) / 256);
        }
        if (fuse_rd) {
            A.zp = lay.s_sorted;  A.zn = e->atom.m * H;  A.n_z = flat_grid(A.zn, 64);
        }
        const dim3 grid(A.n_t + A.n_d + A.n_s[0] + A.n_s[1] + A.n_ss[0] + A.n_ss[1] + A.n_z + A.n_x);
        if (keep_atoms) hipLaunchKernelGGL(k_enc_prologue<true>, grid, dim3(256), 0, S(st), A);
        else hipLaunchKernelGGL(k_enc_prologue<false>, grid, dim3(256), 0, S(st), A);
        FN_TRY(launch_status("fn_encoder_forward: prologue"));
    }

    for (int l = 0; l < e->n_layers; ++l) {
        const LevelView vb = level_view(e, lay, l, LV_BOND), va = level_view(e, lay, l, LV_ATOM), vfb = level_view(e, lay, l, LV_FBOND);
        const LevelView vf = level_view(e, lay, l, LV_FRAG);
        const bool last = l + 1 == e->n_layers;

        float* y_atoms = last ? out_atoms : va.a.y;
        float* y_frags = last ? out_frags : vf.a.y;
        // out_bond / out_fbond == null: the caller reads neither (a finetune head pools atoms and fragments only, gat2.py:816-826): the last
        // layer's activated bond / fragment-bond rows are not stored.  The launches are prepared with a stand-in pointer (shape and instance
        // as with the store) and the epilogue's target is cleared afterwards.
        const bool drop_edge_out = last && out_bond == nullptr;
        float* y_bond = last ? (out_bond ? out_bond : vb.a.raw) : vb.a.y;
        float* y_fbond = last ? (out_fbond ? out_fbond : vfb.a.raw) : vfb.a.y;
        // act(dropout(.)) of the four layer outputs rides in the producing kernels' epilogues
        const fn_act_epilogue ep_atoms = act_epilogue(e, rng, va, y_atoms), ep_frags = act_epilogue(e, rng, vf, y_frags);
        const fn_act_epilogue ep_bond = act_epilogue(e, rng, vb, y_bond), ep_fbond = act_epilogue(e, rng, vfb, y_fbond);
        // L1 bond graph
        const bool fuse_ns = H >= 2;         // a head's columns fit one wave's 64-column half for H >= 2
        auto project = [&](const LevelView& v) -> int {       // a level's projection as a launch of its own
            if (fuse_ns) return launch_linear128_ns(v.x, v.K, v.Wt, v.bias, v.a.h, v.rows, nullptr, node_scalars(v), st);
            FN_TRY(fn_linear128_f32(v.x, v.K, v.Wt, v.bias, v.a.h, v.rows, nullptr, st));
            return fn_node_scalars_f32(v.a.h, v.att, v.att_w, 0, v.src_off, v.s_dst, v.s_src, v.rows, H, st);
        };
        // layers >= 1: the three projections (K = 128) depend only on the previous layer.  With co-launching (FN_TUNE_GEMM_COLAUNCH)
        // the bond / fragment-bond projections already ran beside the previous layer's atom level and the atom projection rides
        // with this layer's bond levels below; otherwise one grouped launch for the three
        const bool grouped = l > 0 && fuse_ns;
        bool atoms_projected = false;
        LinTasks with_pair{};                      // rides with the bond + fragment-bond launch of this layer
        if (grouped && colaunch) {
            with_pair.n = 1;
            with_pair.t[0] = proj_task(va);
        } else if (grouped) {
            LinTasks T{};
            T.n = no_fb ? 2 : 3;
            T.t[0] = proj_task(vb);  T.t[1] = proj_task(va);  T.t[2] = proj_task(vfb);
            FN_TRY(launch_linear128_group(T, S(st)));
        } else if (l == 0 && fuse_ns && !no_fb && vb.K <= 20 && vfb.K <= 20) {
            LinTasks T{};                               // layer 0: both edge-feature projections have K <= 20 -> one launch
            T.n = 2;
            T.t[0] = proj_task(vb, vb.K);  T.t[1] = proj_task(vfb, vfb.K);
            if (colaunch && va.K > 20 && va.K <= 168) {     // the atom features' projection needs nothing of the bond levels either: same launch
                T.t[2] = T.t[1];  T.t[1] = T.t[0];          // its (longer) workgroups first
                T.t[0] = proj_task(va, va.K);
                T.n = 3;
                atoms_projected = true;
            }
            FN_TRY(launch_linear128_small_group(T, S(st)));
        } else {
            FN_TRY(project(vb));
            if (!no_fb) FN_TRY(project(vfb));
        }
        // a level's attention pass, prepared: raw_out = where its raw rows go (null: nobody reads them)
        auto prep = [&](const LevelView& v, float* raw_out, const fn_act_epilogue& ep, GatFwdArgs* A) -> int {
            const fn_edge_term et = fwd_edge_term(v, lay.s_sorted);
            return prep_gat_fwd(v.a.h, v.s_dst, v.s_src, v.att, v.att_w, &et, v.pl, 0.2f, raw_out, v.a.p, nullptr, &ep, H, A, v.a.o2, v.a.sg);
        };
        // ... and what the engine sets on it whether the level runs or not (an absent level of a two-level launch still takes part in
        // the choice of the launch's kind).  p_wanted: a read-out pass keeps the last layer's probabilities: the slots exist in every
        // workspace; same kernel instances, one more store per edge
        const bool keep_p = readout && last;
        auto finish = [&](const LevelView& v, GatFwdArgs* A, bool p_wanted) {
            A->p_edge_major = one ? 1 : 0;
            if (no_bwd && !(keep_p && p_wanted)) A->p_sorted = nullptr;
            A->n_real = v.n_real;
        };
        // L1 bond graph and L4a fragment-bond graph: neither reads the other's output -> one launch for both
        GatFwdArgs gb, gfb{};
        FN_TRY(prep(vb, (no_bwd && fuse_rd && ep_bond.y) ? nullptr : vb.a.raw, ep_bond, &gb));
        // (the raw fragment-bond rows are the fragment graph's edge attribute: read in the last layer only, like the raw atom rows below)
        if (!no_fb) FN_TRY(prep(vfb, (last || !ep_fbond.y) ? vfb.a.raw : nullptr, ep_fbond, &gfb));
        finish(vb, &gb, readout && readout->bonds);
        finish(vfb, &gfb, readout && readout->fbonds);
        if (drop_edge_out) gb.ep.y = gfb.ep.y = nullptr;
        // (evaluation passes only, like FN_TUNE_FWD_BLOCKS_EVAL_LARGE: a training pass gets fewer, longer-lived half-waves from prep_gat_fwd
        // on purpose, and the cap was only ever measured forward-only)
        if (const int tail_rows = tune(FN_TUNE_FWD_TAIL_ROWS); !(ep_fbond.y && ep_fbond.p > 0.f) && tail_rows > 0 && gfb.rows_per_hw > tail_rows) {
            gfb.rows_per_hw = tail_rows;             // (the second level's workgroups start last: short ones)
            gfb.nblk = (int)((e->fbond.n + (int64_t)kRows * tail_rows - 1) / ((int64_t)kRows * tail_rows));
        }
        if (fuse_rd) {
            gb.rd_A = va.att + va.mid_off;  gb.rd_lda = va.att_w;  gb.rd_J = H;  gb.rd_out = lay.s_sorted;  gb.rd_pos = e->atom.inv_d;  gb.rd_m = e->atom.m;
        }
        if (l == 0) FN_TRY(prof_event(0, S(st)));
        if (with_pair.n) {
            FN_TRY(launch_gat_fwd_pair_lin(gb, gfb, with_pair, H, S(st), pm_bonds, pm_fbonds));
        } else {
            FN_TRY(launch_gat_fwd_pair(gb, gfb, H, S(st), pm_bonds, pm_fbonds));
        }
        if (l == 0) FN_TRY(prof_event(1, S(st)));

        // L2 atom graph (+ self loops), edge term = <new_bond, a[:, d:d+128]>
        if (!grouped && !atoms_projected) FN_TRY(project(va));
        if (!fuse_rd) FN_TRY(fn_row_dots_sorted_f32(vb.a.raw, va.att, va.att_w, va.mid_off, H, va.pl, lay.s_sorted, st));
        GatFwdArgs ga;
        if (colaunch && !last) {
            // the next layer's bond / fragment-bond projections read this layer's bond-level outputs, not its atom level: same launch
            LinTasks T{};
            T.n = no_fb ? 1 : 2;
            T.t[0] = proj_task(level_view(e, lay, l + 1, LV_BOND));  T.t[1] = proj_task(level_view(e, lay, l + 1, LV_FBOND));
            // (an inner layer's raw atom rows are read by nobody -- the fragment sums exist in the last layer only -- so only y is stored)
            FN_TRY(prep(va, ep_atoms.y ? nullptr : va.a.raw, ep_atoms, &ga));
            finish(va, &ga, readout && readout->atoms);
            FN_TRY(launch_gat_fwd_lin(ga, T, H, S(st), pm_atoms));
        } else {
            FN_TRY(prep(va, (last || !ep_atoms.y) ? va.a.raw : nullptr, ep_atoms, &ga));
            finish(va, &ga, readout && readout->atoms);
            FN_TRY(launch_gat_fwd(ga, H, S(st), pm_atoms));
        }

        // L3 atom -> fragment sum.  Like L4b below it is only ever read in the last layer (the next layer recomputes its own
        // sum from its own atoms before first use, gat2.py:234), so inner layers skip it too.
        float* frags = vf.a.h;
        const bool tail_mol = last && tail_mol_on(e);      // sums + fragment graph + readout: one molecule-resident launch
        const bool tail_fused = !tail_mol && last && !lite && !edge && H > 1 && e->F > 0 && e->N >= 4 * e->F && e->frag.m > 0 &&
                                !(((uintptr_t)lay.atoms_new | (uintptr_t)frags) & 15);
        if (last && !tail_fused && !tail_mol) FN_TRY(fn_segment_sum_f32(lay.atoms_new, FN_D, e->a2f.rowptr, e->a2f.perm, e->a2f.pos_base, frags, e->F, FN_D, e->N, st));

        // L4b fragment graph on the raw fragment sums.  Only the last layer's result is ever read: the next layer
        // overwrites x_frags with its own atom->fragment sum before first use (gat2.py:234), so inner
        // layers skip this level entirely (the reference computes it and throws it away).
        const fn_edge_term et_f = fwd_edge_term(vf, lay.s_sorted);
        if (last && lite) {      // gat2_lite: the encoder's fragment output is act(dropout(.)) of the plain fragment sums
            FN_TRY(fn_dropout_act_f32(frags, y_frags, e->F * FN_D, p, e->seed, rng.y[l][vf.rng_slot], e->offset_dev, 1, st));
        } else if (last && edge) {   // gat2_edge (gat2_edge.py:148-172): edge term = <Linear(8 -> 128)(cnx_attr), f[:, d:d+128]>, folded in-kernel
            FN_TRY(fn_node_scalars_f32(frags, vf.att, vf.att_w, 0, vf.src_off, vf.s_dst, vf.s_src, e->F, H, st));
            FN_TRY(fn_gat_fwd_f32(frags, vf.s_dst, vf.s_src, vf.att, vf.att_w, &et_f, vf.pl, 0.2f, nullptr, vf.a.p, nullptr, nullptr, nullptr, 0, &ep_frags, H, st));
        } else if (last && tail_mol) {
            FN_TRY(launch_tail_fwd(e, lay, vf, ep_frags, y_atoms, S(st)));
        } else if (last) {
            if (tail_fused) {                                // atom -> fragment sum + node scalars + edge term: one launch
                FragTailArgs T{};
                T.src = lay.atoms_new;  T.rowptr = e->a2f.rowptr;  T.perm = e->a2f.perm;  T.pos_base = e->a2f.pos_base;  T.out = frags;
                T.n_seg = e->F;  T.att = vf.att;  T.att_w = vf.att_w;  T.dst_off = 0;  T.src_off = vf.src_off;  T.s_dst = vf.s_dst;  T.s_src = vf.s_src;
                T.nblk_seg = (int)(e->F < 8 * kGridCap ? e->F : 8 * kGridCap);
                T.feat = vfb.a.raw;  T.A = vf.att;  T.lda = vf.att_w;  T.off = vf.mid_off;  T.pl = e->frag;  T.s_sorted = lay.s_sorted;
                T.nblk_rd = row_grid(e->frag.m, kGridCap);
                const dim3 grid((unsigned)(T.nblk_seg + T.nblk_rd));
                with_const<2, 4, 8>(H, [&](auto h) { hipLaunchKernelGGL((k_frag_tail<FN_CV(h)>), grid, dim3(kBlock), 0, S(st), T); });      // (tail_fused: H > 1)
                FN_TRY(launch_status("fragment tail (sum + node scalars + edge term)"));
            } else {
                FN_TRY(fn_row_dots_sorted_f32(vfb.a.raw, vf.att, vf.att_w, vf.mid_off, H, vf.pl, lay.s_sorted, st));
                FN_TRY(fn_node_scalars_f32(frags, vf.att, vf.att_w, 0, vf.src_off, vf.s_dst, vf.s_src, e->F, H, st));
            }
            FN_TRY(fn_gat_fwd_f32(frags, vf.s_dst, vf.s_src, vf.att, vf.att_w, &et_f, vf.pl, 0.2f, nullptr, vf.a.p, nullptr, nullptr, nullptr, 0, &ep_frags, H, st));
        }
    }
    if (readout) {      // the fragment level stores its probabilities on all three tail paths, under no_backward too (its p above)
        const int l = e->n_layers - 1;
        const Level order[4] = {LV_BOND, LV_FBOND, LV_ATOM, LV_FRAG};
        float* const sums[4] = {readout->bonds, readout->fbonds, readout->atoms, readout->frags};
        fni::AttnReadoutTask tasks[4];
        for (int q = 0; q < 4; ++q) {
            const LevelView v = level_view(e, lay, l, order[q]);
            tasks[q] = fni::AttnReadoutTask{*v.pl, v.a.p, sums[q], v.n_real};
        }
        FN_TRY(fni::launch_attn_readout(tasks, 4, H, S(st)));
    }
    return 0;
}

extern "C" {

int fn_encoder_backward(const fn_encoder* e, const float* out_atoms, const float* out_frags, const float* out_bond,
                        const float* out_fbond, const float* g_atoms, const float* g_frags, const float* g_bond,
                        const float* g_fbond, const fn_layer_weights* grads, float* scratch, int64_t scratch_floats,
                        fn_stream_t st) {
    FN_TRY(enc_check(e));
    if (!grads || !scratch || !out_atoms || !out_frags) return fail(FN_EINVAL, "fn_encoder_backward: null argument");
    if ((g_bond && !out_bond) || (g_fbond && !out_fbond)) return fail(FN_EINVAL, "fn_encoder_backward: a gradient of an output the forward pass did not store (out_bond / out_fbond were null)");
    if (const fn_adam_slice* a = e->adam_rider) {
        if (a->n < 0 || (a->n > 0 && (!a->p || !a->g || !a->m || !a->v || !a->lr_dev || !a->step_dev ||
                                      (((uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v) & 15))))
            return fail(FN_EINVAL, "fn_encoder_backward: bad adam_rider (null or misaligned buffer, or no device step count / learning rate)");
    }
    if (!e->training && e->no_backward != 0)
        return fail(FN_EINVAL, "fn_encoder_backward: the forward pass of this descriptor saved nothing for a backward pass (fn_encoder.no_backward)");
    if (!form_matches_forward(e))
        return fail(FN_EINVAL, "fn_encoder_backward: FN_TUNE_BWD_ONE changed since the forward pass that wrote this workspace");
    const EncLayout lay = enc_layout(e, e->ws, forward_was_gated(e));      // a gated forward: layer 0's weight gradient reads the gated copy
    if (lay.total > e->ws_floats) return fail(FN_EINVAL, "fn_encoder_backward: workspace too small");
    const BwdLayout bw = bwd_layout(e, scratch);
    if (bw.total > scratch_floats) return fail(FN_EINVAL, "fn_encoder_backward: scratch too small");
    const RngPlan rng = rng_plan(e);
    if (e->g_pooled && !tail_mol_on(e)) return fail(FN_EINVAL, "fn_encoder_backward: dL/d(readout) is only taken by the fused fragment tail (fn_encoder_fused_tail)");
    const EncOutputs y{{out_bond, out_atoms, out_fbond, out_frags}}, gy{{g_bond, g_atoms, g_fbond, g_frags}};      // by Level
    if (one_pass_on(e)) return encoder_backward_one(e, lay, bw, rng, y, gy, grads, S(st));
    const int H = e->heads;
    hipStream_t hs = S(st);
    ParamGradQueue rq;
    rq.st = hs;                      // all parameter-gradient reductions run as one launch at the very end, and so do the K = 128
                                     // weight-gradient partial products (ParamGradQueue::wgrad)
    rq.defer_mixed = tune(FN_TUNE_GEMM_COLAUNCH) != 0;      // ... and layer 0's
    rq.rider = e->adam_rider;

    // (This is the general path: any head count, hand-built atom graphs, gat2_edge's fragment graph.  The configurations the one-pass
    // backward covers never get here, so its launches run in plain dependency order: the last layer's gates and fragment levels, then
    // per layer the atom level's two passes, the bond and fragment-bond levels' two passes each, and one grouped launch for the layer's
    // input-gradient products.  The co-launched / pipelined forms of rounds 2-3 are retired: tools/probe/retired/.)
    // ---- through act(dropout(.)): gradients of the pre-activation tensors.  For the last layer they come from the caller's output
    // gradients (and the fragment graph, which only that layer runs: a layer's x_frags input is dead in the reference, overwritten at
    // gat2.py:234); for inner layers the input-gradient GEMMs of layer l+1 write them (mask and ReLU gate fused into their epilogue)
    LastGrads top{};
    FN_TRY(last_layer_output_grads(e, lay, bw, y, gy, grads, rq, false, hs, &top));
    bool have[kLevels] = {top.have[LV_BOND], top.have[LV_ATOM], top.have[LV_FBOND]};      // by Level: g_pre holds layer l's gradient rows

    struct Parts { int n_a = 0, n_e = 0; };
    for (int l = e->n_layers - 1; l >= 0; --l) {
        const LevelView vb = level_view(e, lay, l, LV_BOND), va = level_view(e, lay, l, LV_ATOM), vfb = level_view(e, lay, l, LV_FBOND);
        const LevelScratch &sb = bw.lv[l][LV_BOND], &sa = bw.lv[l][LV_ATOM], &sfb = bw.lv[l][LV_FBOND];
        const fn_layer_weights& g = grads[l];
        // the three input-gradient products of a layer feed layer l-1 only: one grouped launch at the end of the layer.  A product
        // writes dL/d(pre-activation output of the level one layer down), gated by that layer's dropout mask and ReLU
        LinTasks dxT{};
        bool nxt[kLevels] = {false, false, false};     // what this layer hands to layer l-1
        auto input_grad = [&](const LevelView& v, const LevelScratch& sc) {
            const LevelView below = level_view(e, lay, l - 1, v.lv);
            dxT.t[dxT.n++] = LinTask{v.Wt, sc.g_h, v.W, nullptr, bw.g_pre[v.lv], v.rows, act_epilogue(e, rng, below, below.a.y),
                                     NodeScalarEpi{nullptr, nullptr, nullptr, 0, 0, 0, 0}, 0, 0};
            nxt[v.lv] = true;
        };

        // ---- L2 atom graph
        if (have[LV_ATOM]) {
            int n_a = 0, n_e = 0, gr = 0;
            FN_TRY(fn_gat_bwd_dst_f32(bw.g_pre[LV_ATOM], va.a.h, va.a.p, &va.et, va.pl, 0.2f, nullptr, sa.dz, sa.pz, sa.g_s_dst, nullptr, &n_e, H, st));
            // source pass + the edge term <new_bond, a[:, d:d+128]> (dL/dnew_bond accumulates into g_pre of the bonds, dL/da mid block)
            FN_TRY(bwd_src_and_edge_term(va, sa, bw.g_pre[LV_ATOM], sa.g_h, vb.a.raw, bw.g_pre[LV_BOND], have[LV_BOND], &n_a, &gr, hs));
            if (gr) have[LV_BOND] = true;
            FN_TRY(level_params(rq, va, level_weights(g, LV_ATOM), sa, ParamWork{n_a, 0, gr}, hs));
            if (l) input_grad(va, sa);
        }

        // ---- L1 bond graph and L4a fragment-bond graph: both destination passes, then both source passes
        Parts nb, nfb;
        auto dst_pass = [&](const LevelView& v, const LevelScratch& sc, Parts* n) {
            return fn_gat_bwd_dst_f32(bw.g_pre[v.lv], v.a.h, v.a.p, &v.et, v.pl, 0.2f, nullptr, nullptr, sc.pz, sc.g_s_dst, sc.part_e, &n->n_e, H, st);
        };
        auto src_pass = [&](const LevelView& v, const LevelScratch& sc, Parts* n) {
            return engine_bwd_src(v, sc, bw.g_pre[v.lv], sc.g_h, &n->n_a, S(st));
        };
        if (have[LV_BOND]) FN_TRY(dst_pass(vb, sb, &nb));
        if (have[LV_FBOND]) FN_TRY(dst_pass(vfb, sfb, &nfb));
        if (have[LV_BOND]) FN_TRY(src_pass(vb, sb, &nb));
        if (have[LV_FBOND]) FN_TRY(src_pass(vfb, sfb, &nfb));
        // (the fragment-bond level's product and parameter work are queued before the bond level's)
        if (have[LV_FBOND]) {
            if (l) input_grad(vfb, sfb);
            FN_TRY(level_params(rq, vfb, level_weights(g, LV_FBOND), sfb, ParamWork{nfb.n_a, nfb.n_e}, hs));
        }
        if (have[LV_BOND]) {
            FN_TRY(level_params(rq, vb, level_weights(g, LV_BOND), sb, ParamWork{nb.n_a, nb.n_e}, hs));
            if (l) input_grad(vb, sb);
        }
        if (dxT.n) FN_TRY(launch_linear128_group(dxT, hs));
        for (Level v : kProjected) have[v] = nxt[v];
    }
    return rq.flush(true);
}

// the three layer-0 rows of the scratch fn_encoder_backward left behind, times the three layer-0 weights: one launch (input_grad.hip)
int fn_encoder_backward_inputs(const fn_encoder* e, const float* scratch, int64_t scratch_floats, const fn_input_grads* in, fn_stream_t st) {
    FN_TRY(enc_check(e));
    if (!scratch || !in) return fail(FN_EINVAL, "fn_encoder_backward_inputs: null argument");
    if (e->variant == 2) return fail(FN_EUNSUPPORTED, "fn_encoder_backward_inputs: input gradients exist for variants 0 (gat2) and 1 (gat2_lite), not for gat2_edge");
    if (e->variant == 1 && (in->dx_fbonds || in->dots_fbonds))
        return fail(FN_EINVAL, "fn_encoder_backward_inputs: gat2_lite has no fragment-bond level (dx_fbonds / dots_fbonds must be null)");
    if (e->training && e->drop_p > 0.f)
        return fail(FN_EUNSUPPORTED, "fn_encoder_backward_inputs: a training pass with drop_p > 0 (the input dropout's gate on x_atoms would have to be replayed)");
    if (!e->training && e->no_backward != 0)
        return fail(FN_EINVAL, "fn_encoder_backward_inputs: the forward pass of this descriptor saved nothing for a backward pass (fn_encoder.no_backward)");
    if (!form_matches_forward(e))
        return fail(FN_EINVAL, "fn_encoder_backward_inputs: FN_TUNE_BWD_ONE changed since the forward pass that wrote this workspace");
    if (forward_was_gated(e))
        return fail(FN_EUNSUPPORTED, "fn_encoder_backward_inputs: the forward pass ran with an input gate (fn_encoder_forward_keep); there are no input gradients of a masked pass");
    const BwdLayout bw = bwd_layout(e, const_cast<float*>(scratch));
    if (bw.total > scratch_floats) return fail(FN_EINVAL, "fn_encoder_backward_inputs: scratch too small");
    const fn_layer_weights& w0 = e->w[0];
    const fn_linear_dx_task tasks[FN_MAX_DX_TASKS] = {
        {bw.lv[0][LV_ATOM].g_h, w0.proj_a_w, in->dx_atoms, in->delta_atoms, in->dots_atoms, e->N, e->k_atom0, 0},
        {bw.lv[0][LV_BOND].g_h, w0.proj_b_w, in->dx_bonds, in->delta_bonds, in->dots_bonds, e->E, e->k_bond0, 0},
        {bw.lv[0][LV_FBOND].g_h, w0.proj_fb_w, in->dx_fbonds, in->delta_fbonds, in->dots_fbonds, e->variant == 1 ? 0 : e->EF, e->k_fbond0, 0},
    };
    return fni::launch_linear_dx(tasks, FN_MAX_DX_TASKS, S(st));
}

// ---- the operator entry points of the kernel families that live in this unit
int fn_gat_bwd_src_f32(const float* g_out, const float* h, const float* pz_src,
                       const float* g_s_dst, const float* att, int att_w, int dst_off, int src_off,
                       const fn_gat_plan* plan, float* g_h, float* part_a, int* n_part_a, int heads, fn_stream_t stream) {
    GatBwdSrcArgs A;
    if (int rc = prep_gat_bwd_src(g_out, h, pz_src, g_s_dst, att, att_w, dst_off, src_off, plan, g_h, part_a, n_part_a, heads, &A)) return rc;
    return launch_gat_bwd_src(A, heads, S(stream));
}

int fn_sort_edge_attr_f32(const float* x, int K, const fn_gat_plan* plan, float* x_sorted, fn_stream_t stream) {
    if (!plan || K < 1) return fail(FN_EINVAL, "fn_sort_edge_attr_f32: bad argument");
    if (plan->m == 0) return 0;
    if (!x_sorted || (plan->m_real > 0 && !x)) return fail(FN_EINVAL, "fn_sort_edge_attr_f32: null buffer");
    hipLaunchKernelGGL(k_sort_edge_attr, dim3(flat_grid(plan->m * K, kGridCap)), dim3(kBlock), 0, S(stream), x, K, *plan, x_sorted, 0);
    return launch_status("fn_sort_edge_attr_f32");
}
int fn_sort_edge_attr_src_f32(const float* x, int K, const fn_gat_plan* plan, float* x_src, fn_stream_t stream) {
    if (!plan || K < 1) return fail(FN_EINVAL, "fn_sort_edge_attr_src_f32: bad argument");
    if (plan->m == 0) return 0;
    if (!x_src || (plan->m_real > 0 && !x)) return fail(FN_EINVAL, "fn_sort_edge_attr_src_f32: null buffer");
    hipLaunchKernelGGL(k_sort_edge_attr, dim3(flat_grid(plan->m * K, kGridCap)), dim3(kBlock), 0, S(stream), x, K, *plan, x_src, 1);
    return launch_status("fn_sort_edge_attr_src_f32");
}

int fn_row_dots_sorted_bwd_f32(const float* g_s_sorted, const float* feat, const float* A, int lda, int off, int J,
                               const fn_gat_plan* plan, float* g_feat, float* part, int* n_part, fn_stream_t stream) {
    if (!A || !plan || !part || !n_part || J < 1 || J > 8 || ((lda | off) & 3))
        return fail(FN_EINVAL, "fn_row_dots_sorted_bwd_f32: bad argument");
    if (plan->m_real > 0 && (!g_s_sorted || !feat || !g_feat || !plan->inv_d))
        return fail(FN_EINVAL, "fn_row_dots_sorted_bwd_f32: null buffer");
    const int g = row_grid(plan->m_real, kRowDotsBwdBlocks);
    *n_part = g;
    hipLaunchKernelGGL(k_row_dots_sorted_bwd, dim3(g), dim3(kBlock), 0, S(stream),
                       RowDotsBwdArgs{g_s_sorted, feat, A, lda, off, J, *plan, g_feat, part, nullptr, 0, g});
    return launch_status("fn_row_dots_sorted_bwd_f32");
}

}  // extern "C"
