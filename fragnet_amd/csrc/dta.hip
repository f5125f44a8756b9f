// dta.hip -- the drug-target-affinity model's own layers (reference model/dta/model.py, DTAModel2): what sits beside the FragNet encoder.
// A translation unit of its own: nothing of the encoder, of the prediction heads or of cdrp.hip reaches these kernels.
//   * the protein convolution Conv1d(L -> F, KS)(Embedding(V, D)(tok)) along the embedding axis, in its HISTOGRAM form.  The layer is linear
//     in the V-row table E, so with A[b, v, f, k] = sum of W[f, c, k] over the positions c with tok[b, c] = v (a histogram of W over the
//     token values: L F KS adds per sample)
//         conv[b, f, j] = bias[f] + sum_v sum_k A[b, v, f, k] E[v, j + k]                  F J V KS products instead of F J L KS
//     and the backward, g = d loss / d conv:
//         G[b, v, f, k] = sum_j g[b, f, j] E[v, j + k]        dW[f, c, k] = sum_b G[b, tok[b, c], f, k]        dbias[f] = sum_b sum_j g[b, f, j]
//         dE[v, d]      = sum_b sum_f sum_k A[b, v, f, k] g[b, f, d - k]                   (terms with d - k outside [0, J) are absent)
//     A token outside [0, V) falls into no bin and is gathered from nowhere: it never indexes memory.
// Linear(F J, 300) behind it is fn_dense_fwd_f32 / fn_dense_bwd_f32 (dense_head.inc); the pair head fc2(fc1(cat(drug_enc, xt))),
// fn_dta_pair_*, is the <300, false> instance of pair_head.hip.
// Arithmetic: fp32 in, fp32 accumulate, no atomics, every sum over positions, samples or rows in a fixed order.
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

// ---- the built instance of the convolution
constexpr int kF = 32, kKS = 8, kFK = kF * kKS, kVMax = 32;        // a workgroup's 256 (f, k) columns; the token values
constexpr int kLMax = 4096, kDMin = kKS, kDMax = 512;
constexpr int kHistChunks = 4;                                      // position chunks of the histogram kernel: one 256-thread group each
constexpr int kDwCols = 4;                                          // positions per workgroup of the dW gather
constexpr int kDwRows = 32;                                         // samples per part of the dW gather (more than this: partial sums)
constexpr int kDwPartsMax = 16;

// rows of E / of g in LDS: a stride that is a multiple of 4 floats (16-byte reads) and an ODD number of float4 (sixteen lanes that read
// the same column of sixteen consecutive rows hit sixteen different 16-byte slots), long enough for the widest read past the row's end
__host__ __device__ inline int odd_quads(int n) { n = (n + 3) & ~3;  return (n >> 2) & 1 ? n : n + 4; }
__host__ __device__ inline int e_stride(int D) { return odd_quads(((D + 3) & ~3) + 4); }          // reads reach column roundup4(D) + 3
__host__ __device__ inline int g_stride(int D) { return odd_quads(((D + 3) & ~3) + 8); }          // [8 zeros | J values | zeros], reads reach roundup4(D) + 7

// ---- (a) histogram: A[b][v][f k] = sum over c with tok[b, c] = v of W[f, c, k].  One workgroup per sample, 1024 threads = 4 position
// chunks x 256 columns (f, k).  A thread owns ITS column of its chunk's V bins in LDS (no two threads ever touch one word) and walks its
// chunk's positions in order; the four chunks are added in order at the end.  W is read once per sample (1 MB at L = 1000, from L2).
__global__ __launch_bounds__(1024) void k_dta_hist(const long long* __restrict__ tok, const float* __restrict__ W, float* __restrict__ A,
                                                   int L, int V) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* bins = smem;                                             // [kHistChunks][V][256]
    int* stok = reinterpret_cast<int*>(smem + kHistChunks * V * kFK);      // [L]: the token, or -1 outside [0, V)
    const int t = threadIdx.x, col = t & (kFK - 1), q = t >> 8, b = blockIdx.x;
    for (int i = t; i < kHistChunks * V * kFK; i += 1024) bins[i] = 0.f;
    const long long* tp = tok + (size_t)b * L;
    for (int c = t; c < L; c += 1024) {
        const long long v = tp[c];
        stok[c] = v >= 0 && v < V ? (int)v : -1;
    }
    __syncthreads();
    const int per = (L + kHistChunks - 1) / kHistChunks;
    const int c0 = q * per, c1 = min(L, c0 + per);
    float* mine = bins + q * V * kFK + col;
    const float* wp = W + (size_t)(col >> 3) * L * kKS + (col & 7);
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
        const float w = wp[(size_t)c * kKS];
        const int v = stok[c];
        if (v >= 0) mine[v * kFK] += w;
    }
    __syncthreads();
    float* ap = A + (size_t)b * V * kFK;
    for (int i = t; i < V * kFK; i += 1024) {
        float s = bins[i];
#pragma unroll
        for (int r = 1; r < kHistChunks; ++r) s += bins[r * V * kFK + i];
        ap[i] = s;
    }
}

// copies the table E[V][D] into LDS rows of stride Dp, the columns behind D zero
__device__ __forceinline__ void load_table(const float* __restrict__ E, float* __restrict__ sE, int V, int D, int Dp) {
    for (int i = threadIdx.x; i < V * Dp; i += 256) {
        const int v = i / Dp, d = i - v * Dp;
        sE[i] = d < D ? E[(size_t)v * D + d] : 0.f;
    }
}

// ---- (b) contraction: conv[b][f J + j] = bias[f] + sum_v sum_k A[b][v][f k] E[v][j + k].  One workgroup per sample, A[b] and E in LDS.
// A task = one f and four neighbouring j: per v two 16-byte reads of A (the lanes of one f share them), three of E, 32 products.
__global__ __launch_bounds__(256) void k_dta_conv(const float* __restrict__ A, const float* __restrict__ E, const float* __restrict__ bias,
                                                  float* __restrict__ conv, int D, int V) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Dp = e_stride(D), J = D - kKS + 1, nstrip = (J + 3) >> 2, b = blockIdx.x;
    float* sE = smem;                                               // [V][Dp]
    float* sA = smem + V * Dp;                                      // [V][256]
    load_table(E, sE, V, D, Dp);
    const float* ap = A + (size_t)b * V * kFK;
    for (int i = threadIdx.x; i < V * kFK / 4; i += 256) st4(sA + 4 * i, ld4(ap + 4 * i));
    __syncthreads();
    float* out = conv + (size_t)b * kF * J;
    for (int task = threadIdx.x; task < kF * nstrip; task += 256) {
        const int f = task / nstrip, j0 = 4 * (task - f * nstrip);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int v = 0; v < V; ++v) {
            const float4 a0 = ld4(sA + v * kFK + f * kKS), a1 = ld4(sA + v * kFK + f * kKS + 4);
            const float* ep = sE + v * Dp + j0;
            const float4 e0 = ld4(ep), e1 = ld4(ep + 4), e2 = ld4(ep + 8);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float e[12] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w};
#pragma unroll
            for (int k = 0; k < kKS; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(a[k], e[i + k], acc[i]);
        }
        const float bb = bias[f];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (j0 + i < J) out[f * J + j0 + i] = acc[i] + bb;
    }
}

// ---- (c) backward, per sample: G[b] (phase 1: g[b] and E in LDS), then this sample's share of dE and of dbias (phase 2: A[b] takes E's
// place).  g[b] sits in LDS as rows [8 zeros | J values | zeros]: the zeros are the absent terms of dE (d - k < 0 or >= J) and the tail
// of the four-wide j steps of G.
__global__ __launch_bounds__(256) void k_dta_bwd_sample(const float* __restrict__ g, const float* __restrict__ E, const float* __restrict__ A,
                                                        float* __restrict__ G, float* __restrict__ dE_part, float* __restrict__ db_part,
                                                        int D, int V) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int Dp = e_stride(D), Jp = g_stride(D), J = D - kKS + 1, b = blockIdx.x, t = threadIdx.x;
    float* sg = smem;                                               // [F][Jp]
    float* sE = smem + kF * Jp;                                     // [V][Dp], then A[b]: [V][256]
    const float* gp = g + (size_t)b * kF * J;
    for (int i = t; i < kF * Jp; i += 256) {
        const int f = i / Jp, j = i - f * Jp - 8;
        sg[i] = j >= 0 && j < J ? gp[f * J + j] : 0.f;
    }
    load_table(E, sE, V, D, Dp);
    __syncthreads();
    // phase 1: a task = (v, f), eight k; lanes = 32 consecutive f of one v: E is shared, the store is one contiguous run
    const int jsteps = (J + 3) >> 2;
    float* Gp = G + (size_t)b * V * kFK;
    for (int task = t; task < V * kF; task += 256) {
        const int v = task >> 5, f = task & 31;
        const float* ep = sE + v * Dp;
        const float* gr = sg + f * Jp + 8;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < jsteps; ++s) {
            const float4 g4 = ld4(gr + 4 * s), e0 = ld4(ep + 4 * s), e1 = ld4(ep + 4 * s + 4), e2 = ld4(ep + 4 * s + 8);
            const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
            const float e[12] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w, e2.x, e2.y, e2.z, e2.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int k = 0; k < kKS; ++k) acc[k] = fmaf(gv[i], e[i + k], acc[k]);
        }
        st4(Gp + v * kFK + f * kKS, make_float4(acc[0], acc[1], acc[2], acc[3]));
        st4(Gp + v * kFK + f * kKS + 4, make_float4(acc[4], acc[5], acc[6], acc[7]));
    }
    if (t < kF) {                                                   // dbias of this sample: the row's J values in order
        const float* gr = sg + t * Jp + 8;
        float s = 0.f;
        for (int j = 0; j < J; ++j) s += gr[j];
        db_part[(size_t)b * kF + t] = s;
    }
    __syncthreads();
    // phase 2: A[b] over E; a task = (v, four neighbouring d)
    float* sA = sE;
    const float* ap = A + (size_t)b * V * kFK;
    for (int i = t; i < V * kFK / 4; i += 256) st4(sA + 4 * i, ld4(ap + 4 * i));
    __syncthreads();
    const int nstrip = (D + 3) >> 2;
    float* op = dE_part + (size_t)b * V * D;
    for (int task = t; task < V * nstrip; task += 256) {
        const int v = task / nstrip, d0 = 4 * (task - v * nstrip);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int f = 0; f < kF; ++f) {
            const float4 a0 = ld4(sA + v * kFK + f * kKS), a1 = ld4(sA + v * kFK + f * kKS + 4);
            // row position p holds g[f][p - 8]: d - k = d0 + i - k sits at p = d0 + 8 + i - k, i - k in [-7, 3]: positions d0 + 1 .. d0 + 11
            const float* gr = sg + f * Jp + d0;
            const float4 g0 = ld4(gr), g1 = ld4(gr + 4), g2 = ld4(gr + 8);
            const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float w[12] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w, g2.x, g2.y, g2.z, g2.w};
#pragma unroll
            for (int k = 0; k < kKS; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(a[k], w[8 + i - k], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (d0 + i < D) op[v * D + d0 + i] = acc[i];
    }
}

// ---- (d) dW gather: out[p][f][c][k] = sum over the samples b of part p, in order, of G[b][tok[b, c]][f k].  A workgroup = 256 columns
// (f, k) x kDwCols positions x one part of the samples.  One part (M <= kDwRows): out is dW itself.
__global__ __launch_bounds__(256) void k_dta_dw(const long long* __restrict__ tok, const float* __restrict__ G, float* __restrict__ out,
                                                int M, int L, int V, int rows_per_part) {
    const int t = threadIdx.x, c0 = blockIdx.x * kDwCols, p = blockIdx.y;
    const int b0 = p * rows_per_part, b1 = min(M, b0 + rows_per_part);
    float acc[kDwCols];
#pragma unroll
    for (int i = 0; i < kDwCols; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int b = b0; b < b1; ++b) {
        const float* Gp = G + (size_t)b * V * kFK + t;
#pragma unroll
        for (int i = 0; i < kDwCols; ++i) {
            const long long v = c0 + i < L ? tok[(size_t)b * L + c0 + i] : -1;
            if (v >= 0 && v < V) acc[i] += Gp[(int)v * kFK];
        }
    }
    float* op = out + (size_t)p * kF * L * kKS + (size_t)(t >> 3) * L * kKS + (t & 7);
#pragma unroll
    for (int i = 0; i < kDwCols; ++i)
        if (c0 + i < L) op[(size_t)(c0 + i) * kKS] = acc[i];
}

// ---- (e) the sums over samples, in a fixed order.  Workgroups [0, w_blocks): dW = sum of the parts (only with more than one part);
// the next e_blocks: 64 elements of dE each, four sample lanes (b = lane, lane + 4, ..) added through LDS in order; the last: dbias.
__global__ __launch_bounds__(256) void k_dta_combine(const float* __restrict__ dW_part, int n_part, float* __restrict__ dW, int w_quads,
                                                     const float* __restrict__ dE_part, float* __restrict__ dE, int e_elems,
                                                     const float* __restrict__ db_part, float* __restrict__ db, int M, int w_blocks,
                                                     int e_blocks) {
    __shared__ float sm[256];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < w_blocks) {
        const int i = b * 256 + t;
        if (i >= w_quads) return;
        float4 s = ld4(dW_part + 4 * (size_t)i);
        for (int p = 1; p < n_part; ++p) {
            const float4 o = ld4(dW_part + 4 * ((size_t)p * w_quads + i));
            s.x += o.x;  s.y += o.y;  s.z += o.z;  s.w += o.w;
        }
        st4(dW + 4 * (size_t)i, s);
        return;
    }
    if (b < w_blocks + e_blocks) {
        const int e = (b - w_blocks) * 64 + (t & 63), rl = t >> 6;
        float s = 0.f;
        if (e < e_elems)
#pragma unroll 4
            for (int m = rl; m < M; m += 4) s += dE_part[(size_t)m * e_elems + e];
        sm[t] = s;
        __syncthreads();
        if (rl == 0 && e < e_elems) dE[e] = ((sm[t] + sm[t + 64]) + sm[t + 128]) + sm[t + 192];
        return;
    }
    if (t < kF) {
        float s = 0.f;
        for (int m = 0; m < M; ++m) s += db_part[(size_t)m * kF + t];
        db[t] = s;
    }
}

// ---- host side
bool conv_instance_ok(int64_t V, int64_t F, int64_t KS) { return F == kF && KS == kKS && V >= 1 && V <= kVMax; }
int conv_unsupported() {
    return fail(FN_EUNSUPPORTED, "fn_dta_conv_*_f32: the protein convolution is built for F = 32 filters, KS = 8 and V <= 32 token values; other shapes are not built");
}
bool conv_dims_ok(int64_t M, int64_t L, int64_t D) { return M >= 0 && M <= FN_DENSE_MAX_ROWS && L >= 1 && L <= kLMax && D >= kDMin && D <= kDMax; }
int conv_dims_bad(const char* what) { return fail(FN_EINVAL, what); }
int64_t up4(int64_t n) { return (n + 3) & ~(int64_t)3; }
int dw_parts(int64_t M) { return (int)((M + kDwRows - 1) / kDwRows < kDwPartsMax ? (M + kDwRows - 1) / kDwRows : kDwPartsMax); }
}  // namespace

extern "C" {

int fn_dta_conv_fwd_f32(const int64_t* tok, const float* E, const float* W, const float* bias, float* A, float* conv, int64_t M, int64_t L,
                        int64_t D, int64_t V, int64_t F, int64_t KS, fn_stream_t stream) {
    if (!conv_instance_ok(V, F, KS)) return conv_unsupported();
    if (!conv_dims_ok(M, L, D)) return conv_dims_bad("fn_dta_conv_fwd_f32: 0 <= M <= FN_DENSE_MAX_ROWS, 1 <= L <= 4096, 8 <= D <= 512 (any D in that range)");
    if (M == 0) return 0;
    if (!tok || !E || !W || !bias || !A || !conv || misaligned(7, tok) || misaligned(3, E, W, bias, conv) || misaligned(15, A))
        return fail(FN_EINVAL, "fn_dta_conv_fwd_f32: null or misaligned buffer (A: 16 bytes)");
    const size_t lds_h = ((size_t)kHistChunks * V * kFK + L) * sizeof(float);
    FN_TRY(allow_lds(k_dta_hist, lds_h));
    hipLaunchKernelGGL(k_dta_hist, dim3((unsigned)M), dim3(1024), lds_h, S(stream), reinterpret_cast<const long long*>(tok), W, A, (int)L, (int)V);
    FN_TRY(launch_status("fn_dta_conv_fwd_f32 (histogram)"));
    const size_t lds_c = ((size_t)V * e_stride((int)D) + (size_t)V * kFK) * sizeof(float);
    FN_TRY(allow_lds(k_dta_conv, lds_c));
    hipLaunchKernelGGL(k_dta_conv, dim3((unsigned)M), dim3(256), lds_c, S(stream), A, E, bias, conv, (int)D, (int)V);
    return launch_status("fn_dta_conv_fwd_f32");
}

int64_t fn_dta_conv_bwd_ws(int64_t M, int64_t L, int64_t D, int64_t V) {
    if (M <= 0 || L <= 0 || D <= 0 || V <= 0) return 0;
    const int parts = dw_parts(M);
    return M * V * kFK + up4(M * V * D) + up4(M * kF) + (parts > 1 ? (int64_t)parts * kF * L * kKS : 0);
}

int fn_dta_conv_bwd_f32(const float* g_conv, const int64_t* tok, const float* E, const float* A, float* dW, float* dbias, float* dE, float* ws,
                        int64_t M, int64_t L, int64_t D, int64_t V, int64_t F, int64_t KS, fn_stream_t stream) {
    if (!conv_instance_ok(V, F, KS)) return conv_unsupported();
    if (!conv_dims_ok(M, L, D)) return conv_dims_bad("fn_dta_conv_bwd_f32: 0 <= M <= FN_DENSE_MAX_ROWS, 1 <= L <= 4096, 8 <= D <= 512 (any D in that range)");
    if (!dW || !dbias || !dE || (M > 0 && (!g_conv || !tok || !E || !A || !ws)) || misaligned(7, tok) || misaligned(3, g_conv, E, dbias, dE) ||
        misaligned(15, A, dW, ws))
        return fail(FN_EINVAL, "fn_dta_conv_bwd_f32: null or misaligned buffer (A, dW, ws: 16 bytes)");
    if (M == 0) {                                         // no samples: the sums are empty
        FN_TRY(zero_async(dW, kF * L * kKS, stream, "fn_dta_conv_bwd_f32 (no rows)"));
        FN_TRY(zero_async(dbias, kF, stream, "fn_dta_conv_bwd_f32 (no rows)"));
        FN_TRY(zero_async(dE, V * D, stream, "fn_dta_conv_bwd_f32 (no rows)"));
        return 0;
    }
    float* G = ws;
    float* dE_part = G + M * V * kFK;
    float* db_part = dE_part + up4(M * V * D);
    float* dW_part = db_part + up4(M * kF);
    const int parts = dw_parts(M), rows_per_part = (int)((M + parts - 1) / parts);
    const int Dp = e_stride((int)D), Jp = g_stride((int)D);
    const size_t lds = ((size_t)kF * Jp + (size_t)V * (Dp > kFK ? Dp : kFK)) * sizeof(float);
    FN_TRY(allow_lds(k_dta_bwd_sample, lds));
    hipLaunchKernelGGL(k_dta_bwd_sample, dim3((unsigned)M), dim3(256), lds, S(stream), g_conv, E, A, G, dE_part, db_part, (int)D, (int)V);
    FN_TRY(launch_status("fn_dta_conv_bwd_f32 (per sample)"));
    hipLaunchKernelGGL(k_dta_dw, dim3((unsigned)((L + kDwCols - 1) / kDwCols), (unsigned)parts), dim3(256), 0, S(stream),
                       reinterpret_cast<const long long*>(tok), G, parts > 1 ? dW_part : dW, (int)M, (int)L, (int)V, rows_per_part);
    FN_TRY(launch_status("fn_dta_conv_bwd_f32 (dW gather)"));
    const int w_quads = (int)(kF * L * kKS / 4), w_blocks = parts > 1 ? (w_quads + 255) / 256 : 0, e_elems = (int)(V * D), e_blocks = (e_elems + 63) / 64;
    hipLaunchKernelGGL(k_dta_combine, dim3((unsigned)(w_blocks + e_blocks + 1)), dim3(256), 0, S(stream), dW_part, parts, dW, w_quads, dE_part, dE,
                       e_elems, db_part, dbias, (int)M, w_blocks, e_blocks);
    return launch_status("fn_dta_conv_bwd_f32");
}
}  // extern "C"
