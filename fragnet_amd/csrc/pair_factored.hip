// pair_factored.hip -- the pair head of pair_head.hip on a FACTORED batch: U distinct drug rows D[U,256], C distinct second rows S[C,K1] and
// two pair lists pd[M], ps[M] instead of M duplicated rows.  There is nothing between the two Linears, so with W1 = [W1d | W1s],
// A = D W1d^T [U,128], B = S W1s^T [C,128]:
//   out[m]   = alpha[pd[m]] + beta[ps[m]] + (b1 . w2 + b2),    alpha = A w2, beta = B w2
//   g[m]     = 2 (out[m] - y[m]) / M
//   sd[u]    = sum of g over the pairs of drug u,  ss[c] likewise,  G = sum_m g[m]
//   g_D[u,:] = sd[u] v_d,  g_S[c,:] = ss[c] v_s,  v = W1^T w2      (GATE: g_S zeroed where S <= 0, the ReLU that produced S)
//   dW1[j,k] = w2[j] [D^T sd | S^T ss][k],  db1 = w2 G,  db2 = G,  dW2[j] = sum_u sd[u] A[u,j] + sum_c ss[c] B[c,j] + G b1[j]
// Nothing of size M x 128 or M x 256 exists; a pair costs a few scalars.  The same two instances as pair_head.hip and no other:
// <256, gated> (fn_cdrp_pair_factored_*), <300, not gated> (fn_dta_pair_factored_*; 300 = 18 x 16 + 12, the last MFMA step masked).
// Arithmetic as there: fp32 in, fp32 accumulate, v_mfma_f32_16x16x4_f32 for A and B, no float atomics, every sum over pairs or rows in a
// fixed order (the one integer atomic is the forward's arrival counter).  A pair-list value is range-tested before it indexes anything:
// a pair outside [0,U) x [0,C) gets out = 0, g = 0 and adds nothing to the loss or to a gradient.
// Orders of additions: v = W1^T w2 and the last workgroup's sums (dW2, db2, the loss) are pair_bodies.inc's, shared with pair_head.hip; the
// tile-row dot with w2 and the end of a dW1 column block are written here and, the same statements, in pair_head.hip (why:
// pair_bodies.inc); this unit's own are the per-row sums of g over the pair orderings (pf_sigma), the forward's one loss partial and
// the grid's dot, which reads global memory.
// For a step over static capacities (graphstep.FactoredPairGraphedTrainStep): fn_pair_orderings_i32 builds both sides' orderings in one
// launch under a device-side count of the real pairs (k_pair_orderings: integers only, a sort of distinct keys), and
// fn_*_pair_factored_fwd_rows_f32 is the forward under the same count; the backward is the one above, without a count.
#include <stdint.h>
#include <stdio.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

#include "pair_bodies.inc"
constexpr int kTileRows = 16, kSegRows = 64;

// one 16 x 128 tile of X[N,K] Wh^T (Wh = the K columns of W1 at `wcol`, rows LD long) into sh and into P[N,128]: wave w the 32 columns
// [32 w, +32), K in steps of 16 of which the last is masked where K is no multiple of 16
template <int K, int LD>
__device__ __forceinline__ void pf_tile(const float* __restrict__ X, const float* __restrict__ W1, int wcol, int N, int i0,
                                        float (*sh)[kHid + 1], float* __restrict__ P) {
    constexpr int kfull = K & ~15;
    const int l = threadIdx.x & 63, n = l & 15, gq = l >> 4, wv = threadIdx.x >> 6, j0 = wv * 32;
    const int row = min(i0 + n, N - 1);
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    const float* xp = X + (size_t)row * K + 4 * gq;
    const float* wp0 = W1 + (size_t)(j0 + n) * LD + wcol + 4 * gq;
    const float* wp1 = wp0 + (size_t)16 * LD;
#pragma unroll 2
    for (int k0 = 0; k0 < kfull; k0 += 16) pair_step(xp + k0, wp0 + k0, wp1 + k0, true, acc0, acc1);
    if constexpr (kfull < K) pair_step(xp + kfull, wp0 + kfull, wp1 + kfull, kfull + 4 * gq < K, acc0, acc1);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = j0 + 16 * u + n;
        const f32x4 acc = u ? acc1 : acc0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * gq + e;
            sh[r][col] = acc[e];
            if (i0 + r < N) P[(size_t)(i0 + r) * kHid + col] = acc[e];
        }
    }
}

// forward, one launch.  Workgroups [0, nbU): 16 rows of A and their alpha; the next nbC: 16 rows of B and their beta.  Each publishes its
// rows (agent-scope release, then one relaxed add on the arrival counter, which the host zeroes in front of the launch); the workgroup
// that arrives last acquires and writes out[M] and, with a target, g[M] and the one loss partial (already divided by M).
// real_pairs (nullable; fn_*_pair_factored_fwd_rows_f32): the int32 word a static-shape step's staging launch writes (FN_STAGE_COUNT),
// n = *real_pairs clamped to [0, M].  The mean is then over the first n pairs: g = 2 (out - y) / n and the partial is divided by n; behind
// them out = 0, g = 0 exactly, no share of the loss, and the pair lists are not read; n = 0: nothing is divided.  The backward needs no
// count: with orderings of the first n pairs (k_pair_orderings) a padding pair is in no segment, a distinct row without a real pair has
// sigma = 0 -- g_D / g_S exact zeros -- and adds 0 * x to dW1 and dW2, in the same lane at the same place of the same sums.
template <int K1>
__global__ __launch_bounds__(256) void k_pairf_fwd(const float* __restrict__ D, const float* __restrict__ Sx, const int64_t* __restrict__ pd,
                                                   const int64_t* __restrict__ ps, const float* __restrict__ W1, const float* __restrict__ b1,
                                                   const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ target,
                                                   float* __restrict__ A, float* __restrict__ B, float* ab, unsigned* counter,
                                                   float* __restrict__ out, float* __restrict__ g, float* __restrict__ loss_part, int M, int U,
                                                   int C, int nbU, const int* __restrict__ real_pairs) {
    constexpr int kInT = kIn0 + K1;
    __shared__ float sh[kTileRows][kHid + 1];
    __shared__ float sred[256];
    __shared__ unsigned s_ticket;
    const int t = threadIdx.x, b = blockIdx.x;
    const bool first = b < nbU;
    const int i0 = (first ? b : b - nbU) * kTileRows, N = first ? U : C;
    if (first) pf_tile<kIn0, kInT>(D, W1, 0, U, i0, sh, A);
    else pf_tile<K1, kInT>(Sx, W1, kIn0, C, i0, sh, B);
    __syncthreads();
    {
        const int r = t >> 4, sub = t & 15;
        float s = 0.f;                                               // the tile-row dot: the same statements, the same order as k_pair_fwd's
#pragma unroll
        for (int c = 0; c < kHid / 16; ++c) s = fmaf(sh[r][sub + 16 * c], w2[sub + 16 * c], s);
        s += __shfl_xor(s, 8);  s += __shfl_xor(s, 4);  s += __shfl_xor(s, 2);  s += __shfl_xor(s, 1);
        if (sub == 0 && i0 + r < N) ab[(first ? 0 : U) + i0 + r] = s;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_ticket = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        float c0 = 0.f;
        for (int j = 0; j < kHid; ++j) c0 = fmaf(b1[j], w2[j], c0);
        sred[0] = c0 + b2[0];
    }
    __syncthreads();
    const float cst = sred[0];
    __syncthreads();
    const int nr = real_pairs ? min(max(*real_pairs, 0), M) : M;    // pairs the loss is a mean over: all of them without a count
    float d2 = 0.f;
    for (int m = t; m < M; m += 256) {
        float o = 0.f, gm = 0.f;
        if (m < nr) {                                                // behind the count the pair lists are not read
            const int64_t u = pd[m], c = ps[m];
            if (u >= 0 && u < U && c >= 0 && c < C) {
                o = ab[u] + ab[U + c] + cst;
                if (target) {
                    const float d = o - target[m];
                    gm = 2.f * d / (float)nr;
                    d2 += d * d;
                }
            }
        }
        out[m] = o;
        if (target) g[m] = gm;
    }
    if (!target) return;
    sred[t] = d2;
    __syncthreads();
    if (t == 0) {
        float s = sred[0];
        for (int q = 1; q < 256; ++q) s += sred[q];
        loss_part[0] = nr > 0 ? s / (float)nr : 0.f;
    }
}

// sig[r] = the sum of g over the pairs of row base + r, r < 64: 4 lanes per row walk the row's segment of the ordering (ascending pair
// index), added ((0 + 1) + (2 + 3)).  rowptr and perm are range-tested; a row without pairs gives exactly 0.  The caller barriers.
__device__ __forceinline__ void pf_sigma(const float* __restrict__ g, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ perm, int N,
                                         int M, int base, float* sig) {
    const int r = threadIdx.x >> 2, sub = threadIdx.x & 3, row = base + r;
    float s = 0.f;
    if (row < N) {
        const int beg = min(max(rowptr[row], 0), M), end = min(max(rowptr[row + 1], beg), M);
        for (int i = beg + sub; i < end; i += 4) {
            const int p = perm[i];
            if ((unsigned)p < (unsigned)M) s += g[p];
        }
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (sub == 0) sig[r] = s;
}

// backward, one launch.  Workgroups [0, rbU): 64 rows of g_D; the next rbC: 64 rows of g_S (v's half recomputed per workgroup); the next
// ceil((256 + K1) / 16): 16 columns of [D^T sd | S^T ss] over all rows (64 row lanes, added through LDS in order) and their 128 x 16
// block of dW1; the last: dW2, db2, db1 and, with loss != null, loss[0] = the sum of the forward's partials.
template <int K1, bool GATE>
__global__ __launch_bounds__(256) void k_pairf_bwd(const float* __restrict__ g, const float* __restrict__ D, const float* __restrict__ Sx,
                                                   const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ W1,
                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                   const int32_t* __restrict__ rp_d, const int32_t* __restrict__ pm_d,
                                                   const int32_t* __restrict__ rp_s, const int32_t* __restrict__ pm_s, float* __restrict__ g_D,
                                                   float* __restrict__ g_S, float* __restrict__ dW1, float* __restrict__ db1,
                                                   float* __restrict__ dW2, float* __restrict__ db2, const float* __restrict__ loss_part,
                                                   int n_part, float* __restrict__ loss, int M, int U, int C, int rbU, int rbC) {
    constexpr int kInT = kIn0 + K1;
    static_assert(K1 % 4 == 0 && K1 <= 1024, "float4 columns; v's half fits the LDS array");
    __shared__ __attribute__((aligned(16))) float sm[1024 + 16];
    __shared__ float sig[kSegRows];
    __shared__ float s1[1];
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < rbU + rbC) {
        const bool first = b < rbU;
        const int base = (first ? b : b - rbU) * kSegRows, N = first ? U : C, Kx = first ? kIn0 : K1, k0 = first ? 0 : kIn0;
        for (int k = t; k < Kx; k += 256) sm[k] = pair_v<kInT>(w2, W1, k0 + k);
        pf_sigma(g, first ? rp_d : rp_s, first ? pm_d : pm_s, N, M, base, sig);
        __syncthreads();
        const int q4 = Kx / 4;
        float* go = first ? g_D : g_S;
        for (int e = t; e < kSegRows * q4; e += 256) {
            const int r = e / q4, k = 4 * (e % q4), row = base + r;
            if (row >= N) break;
            const float s = sig[r];
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (s != 0.f) {
                o = make_float4(s * sm[k], s * sm[k + 1], s * sm[k + 2], s * sm[k + 3]);
                if (GATE && !first) o = relu_gate4(o, ld4(Sx + (size_t)row * K1 + k));
            }
            st4(go + (size_t)row * Kx + k, o);
        }
        return;
    }
    if (b < rbU + rbC + kPairColBlocks<K1>) {
        const int c4 = t & 3, rl = t >> 2;
        const int col = (b - rbU - rbC) * 16 + 4 * c4;               // of [D | S]; 256 = 16 blocks: a block's columns lie in one half
        const bool first = col < kIn0;
        const bool ok = kInT % 16 == 0 || col < kInT;
        const float* x = first ? D + col : Sx + (col - kIn0);
        const int ldx = first ? kIn0 : K1, N = first ? U : C;
        const int32_t* rp = first ? rp_d : rp_s;
        const int32_t* pm = first ? pm_d : pm_s;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = 0; base < N; base += kSegRows) {              // `first` is uniform over the workgroup: so is the trip count
            pf_sigma(g, rp, pm, N, M, base, sig);
            __syncthreads();
            if (ok && base + rl < N) fma4(acc, sig[rl], ld4(x + (size_t)(base + rl) * ldx));
            __syncthreads();
        }
        st4(sm + 4 * (rl * 4 + c4), acc);                            // from here: the same statements, the same order as k_pair_bwd's
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
    {                                                                 // dW2: 32 float4 columns x 8 row lanes, the rows of A, then of B
        const int c4 = t & 31, rl = t >> 5;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int base = 0; base < U; base += kSegRows) {
            pf_sigma(g, rp_d, pm_d, U, M, base, sig);
            __syncthreads();
            for (int r = rl; r < kSegRows && base + r < U; r += 8) fma4(acc, sig[r], ld4(A + (size_t)(base + r) * kHid + 4 * c4));
            __syncthreads();
        }
        for (int base = 0; base < C; base += kSegRows) {
            pf_sigma(g, rp_s, pm_s, C, M, base, sig);
            __syncthreads();
            for (int r = rl; r < kSegRows && base + r < C; r += 8) fma4(acc, sig[r], ld4(B + (size_t)(base + r) * kHid + 4 * c4));
            __syncthreads();
        }
        pair_last_tail(acc, sm, s1, g, M, w2, loss_part, n_part, loss, db1, dW2, db2,
                       [b1](float s, int j, float G) { return fmaf(G, b1[j], s); });      // G = db2
    }
}

// grid: out[u, c] = D[u] . v_d + S[c] . v_s + (b1 . w2 + b2) for every (u, c), v = W1^T w2 recomputed per workgroup.  A workgroup =
// 16 drug rows (16 lanes each, added across the lanes in a fixed order) x 256 second rows (one thread each).
template <int K1>
__global__ __launch_bounds__(256) void k_pairf_grid(const float* __restrict__ D, const float* __restrict__ Sx, const float* __restrict__ W1,
                                                    const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                    float* __restrict__ out, int U, int C) {
    constexpr int kInT = kIn0 + K1;
    __shared__ __attribute__((aligned(16))) float sv[kInT];
    __shared__ float sa[kTileRows + 1];
    const int t = threadIdx.x, c = blockIdx.x * 256 + t, u0 = blockIdx.y * kTileRows;
    for (int k = t; k < kInT; k += 256) sv[k] = pair_v<kInT>(w2, W1, k);
    if (t == 0) {
        float c0 = 0.f;
        for (int j = 0; j < kHid; ++j) c0 = fmaf(b1[j], w2[j], c0);
        sa[kTileRows] = c0 + b2[0];
    }
    __syncthreads();
    {
        const int r = t >> 4, sub = t & 15, row = min(u0 + r, U - 1);
        float s = 0.f;
#pragma unroll 4
        for (int q = 0; q < kIn0 / 16; ++q) s = fmaf(D[(size_t)row * kIn0 + sub + 16 * q], sv[sub + 16 * q], s);
        s += __shfl_xor(s, 8);  s += __shfl_xor(s, 4);  s += __shfl_xor(s, 2);  s += __shfl_xor(s, 1);
        if (sub == 0) sa[r] = s;
    }
    __syncthreads();
    if (c >= C) return;
    float bt = 0.f;
    for (int k = 0; k < K1; k += 4) {
        const float4 x = ld4(Sx + (size_t)c * K1 + k);
        bt = fmaf(x.x, sv[kIn0 + k], bt);  bt = fmaf(x.y, sv[kIn0 + k + 1], bt);
        bt = fmaf(x.z, sv[kIn0 + k + 2], bt);  bt = fmaf(x.w, sv[kIn0 + k + 3], bt);
    }
    bt += sa[kTileRows];
    for (int r = 0; r < kTileRows && u0 + r < U; ++r) out[(size_t)(u0 + r) * C + c] = sa[r] + bt;
}

// the pair orderings of both sides in one launch (ops.pair_orderings is the reference): workgroup 0 the drug list, workgroup 1 the second's.
// Pair m < n (n = *real_pairs clamped to [0, M]; all M without a count) whose value v lies in [0, N) -- tested as int64, before it is
// narrowed -- gets the key (v << 12 | m) < 2^24; every other position m < M gets (2^24 | m), and the tail up to the power of two P gets
// all ones.  The keys are distinct, so their ascending order is unique: a bitonic network in LDS (P <= 4096 words) sorts them, and
// nothing depends on the order in which anything lands -- there is no atomic.  perm[i] = the key's low 12 bits where it is < 2^24, else
// -1; rowptr[r] = the number of keys below (r << 12), by binary search, r = 0 .. N (N << 12 <= 2^24: rowptr[N] counts the in-range pairs).
// Behind n the pair lists are not read.
constexpr int kOrdThreads = 1024, kOrdShift = 12, kOrdMax = 1 << kOrdShift;
static_assert(FN_DENSE_MAX_ROWS <= kOrdMax, "a row and a pair index share a 24-bit key");
__global__ __launch_bounds__(kOrdThreads) void k_pair_orderings(const int64_t* __restrict__ pd, const int64_t* __restrict__ ps,
                                                                const int* __restrict__ real_pairs, int32_t* __restrict__ rp_d,
                                                                int32_t* __restrict__ pm_d, int32_t* __restrict__ rp_s,
                                                                int32_t* __restrict__ pm_s, int M, int U, int C, int P) {
    __shared__ uint32_t key[kOrdMax];
    const int t = threadIdx.x;
    const bool first = blockIdx.x == 0;
    const int64_t* __restrict__ pl = first ? pd : ps;
    int32_t* __restrict__ rp = first ? rp_d : rp_s;
    int32_t* __restrict__ pm = first ? pm_d : pm_s;
    const int N = first ? U : C;
    const int n = real_pairs ? min(max(*real_pairs, 0), M) : M;
    constexpr uint32_t kOut = 1u << (2 * kOrdShift);
    for (int i = t; i < P; i += kOrdThreads) {
        uint32_t k = 0xffffffffu;
        if (i < M) {
            k = kOut | (uint32_t)i;
            if (i < n) {
                const int64_t v = pl[i];
                if (v >= 0 && v < (int64_t)N) k = ((uint32_t)v << kOrdShift) | (uint32_t)i;
            }
        }
        key[i] = k;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < (P >> 1); i += kOrdThreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                const uint32_t a = key[lo], b = key[hi];
                if ((a > b) == ((lo & k) == 0)) { key[lo] = b;  key[hi] = a; }
            }
            __syncthreads();
        }
    for (int i = t; i < M; i += kOrdThreads) {
        const uint32_t k = key[i];
        pm[i] = k < kOut ? (int32_t)(k & (kOrdMax - 1)) : -1;
    }
    for (int r = t; r <= N; r += kOrdThreads) {
        const uint32_t want = (uint32_t)r << kOrdShift;
        int lo = 0, hi = P;                                          // the first position whose key is >= want
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        rp[r] = min(lo, M);
    }
}

// ---- host side (fail_at, check_widths, zero_param_grads: pair_bodies.inc)
int check_counts(const char* who, int64_t M, int64_t U, int64_t C) {
    if (M < 0 || M > FN_DENSE_MAX_ROWS || U < 0 || U > FN_DENSE_MAX_ROWS || C < 0 || C > FN_DENSE_MAX_ROWS)
        return fail_at(FN_EINVAL, who, "0 <= M, U, C <= FN_DENSE_MAX_ROWS");
    return 0;
}
int64_t factored_ws(int64_t U, int64_t C) { return U < 0 || C < 0 ? 0 : U + C + 4; }      // alpha[U], beta[C], the arrival counter

template <int K1>
int pairf_fwd(const char* who, const float* D, const float* Sx, const int64_t* pd, const int64_t* ps, const float* W1, const float* b1,
              const float* w2, const float* b2, const float* target, float* A, float* B, float* ws, float* out, float* g, float* loss_part,
              int64_t M, int64_t U, int64_t C, int64_t Kd, int64_t K, int64_t H, int64_t Co, const int32_t* real_pairs, fn_stream_t stream) {
    FN_TRY(check_widths<K1>("pair_factored_*", Kd, K, H, Co));
    FN_TRY(check_counts(who, M, U, C));
    if (real_pairs && (!target || ((uintptr_t)real_pairs & 3)))
        return fail_at(FN_EINVAL, who, "a real-pair count goes with a target (and is an aligned int32)");
    if (M == 0) return 0;
    if (U == 0 || C == 0) return fail_at(FN_EINVAL, who, "pairs (M > 0) need U >= 1 and C >= 1");
    if (!D || !Sx || !pd || !ps || !W1 || !b1 || !w2 || !b2 || !A || !B || !ws || !out || (target && (!g || !loss_part)) ||
        misaligned(15, D, Sx, W1) || misaligned(7, pd, ps) || misaligned(3, ws))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    unsigned* counter = reinterpret_cast<unsigned*>(ws + U + C);
    if (hipMemsetAsync(counter, 0, sizeof(unsigned), S(stream)) != hipSuccess) return launch_status(who);
    const int nbU = (int)((U + kTileRows - 1) / kTileRows), nbC = (int)((C + kTileRows - 1) / kTileRows);
    hipLaunchKernelGGL(k_pairf_fwd<K1>, dim3((unsigned)(nbU + nbC)), dim3(256), 0, S(stream), D, Sx, pd, ps, W1, b1, w2, b2, target, A, B, ws,
                       counter, out, g, loss_part, (int)M, (int)U, (int)C, nbU, real_pairs);
    return launch_status(who);
}

template <int K1, bool GATE>
int pairf_bwd(const char* who, const float* g, const float* D, const float* Sx, const float* A, const float* B, const float* W1,
              const float* b1, const float* w2, const int32_t* rp_d, const int32_t* pm_d, const int32_t* rp_s, const int32_t* pm_s,
              float* g_D, float* g_S, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss,
              int64_t M, int64_t U, int64_t C, int64_t Kd, int64_t K, int64_t H, int64_t Co, fn_stream_t stream) {
    FN_TRY(check_widths<K1>("pair_factored_*", Kd, K, H, Co));
    FN_TRY(check_counts(who, M, U, C));
    if (n_part < 0 || n_part > INT32_MAX) return fail_at(FN_EINVAL, who, "n_part out of range");
    if (!W1 || !b1 || !w2 || !dW1 || !db1 || !dW2 || !db2 || (U > 0 && !g_D) || (C > 0 && !g_S) ||
        (M > 0 && (!g || !D || !Sx || !A || !B || !rp_d || !pm_d || !rp_s || !pm_s)) || (loss && n_part > 0 && !loss_part) ||
        misaligned(15, D, Sx, A, B) || misaligned(15, g_D, g_S, dW1) || misaligned(3, rp_d, pm_d, rp_s, pm_s))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    if (M == 0 || U == 0 || C == 0) {                     // no pairs: the sums are empty
        char where[96];
        snprintf(where, sizeof(where), "%s (no pairs)", who);
        if (U > 0) FN_TRY(zero_async(g_D, U * kIn0, stream, where));
        if (C > 0) FN_TRY(zero_async(g_S, C * K1, stream, where));
        return zero_param_grads<K1>(dW1, db1, dW2, db2, loss, stream, where);
    }
    const int rbU = (int)((U + kSegRows - 1) / kSegRows), rbC = (int)((C + kSegRows - 1) / kSegRows);
    hipLaunchKernelGGL((k_pairf_bwd<K1, GATE>), dim3((unsigned)(rbU + rbC + kPairColBlocks<K1> + 1)), dim3(256), 0, S(stream), g, D, Sx, A, B, W1, b1,
                       w2, rp_d, pm_d, rp_s, pm_s, g_D, g_S, dW1, db1, dW2, db2, loss_part, (int)n_part, loss, (int)M, (int)U, (int)C, rbU, rbC);
    return launch_status(who);
}

template <int K1>
int pairf_grid(const char* who, const float* D, const float* Sx, const float* W1, const float* b1, const float* w2, const float* b2, float* out,
               int64_t U, int64_t C, int64_t Kd, int64_t K, int64_t H, int64_t Co, fn_stream_t stream) {
    FN_TRY(check_widths<K1>("pair_factored_*", Kd, K, H, Co));
    FN_TRY(check_counts(who, 0, U, C));
    if (U == 0 || C == 0) return 0;
    if (!D || !Sx || !W1 || !b1 || !w2 || !b2 || !out || misaligned(15, Sx) || misaligned(3, D, W1, out))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    hipLaunchKernelGGL(k_pairf_grid<K1>, dim3((unsigned)((C + 255) / 256), (unsigned)((U + kTileRows - 1) / kTileRows)), dim3(256), 0, S(stream),
                       D, Sx, W1, b1, w2, b2, out, (int)U, (int)C);
    return launch_status(who);
}
}  // namespace

extern "C" {

int fn_pair_orderings_i32(const int64_t* pair_drug, const int64_t* pair_second, const int32_t* real_pairs, int32_t* rowptr_drug,
                          int32_t* perm_drug, int32_t* rowptr_second, int32_t* perm_second, int64_t M, int64_t U, int64_t Cn,
                          fn_stream_t stream) {
    const char* who = "fn_pair_orderings_i32";
    if (M < 0 || M > FN_DENSE_MAX_ROWS || U < 0 || U > FN_DENSE_MAX_ROWS || Cn < 0 || Cn > FN_DENSE_MAX_ROWS)
        return fail_at(FN_EINVAL, who, "0 <= M, U, C <= FN_DENSE_MAX_ROWS");
    if (!rowptr_drug || !rowptr_second || (M > 0 && (!pair_drug || !pair_second || !perm_drug || !perm_second)) ||
        misaligned(7, pair_drug, pair_second) || misaligned(3, rowptr_drug, perm_drug, rowptr_second, perm_second) ||
        ((uintptr_t)real_pairs & 3))
        return fail_at(FN_EINVAL, who, "null or misaligned buffer");
    int P = 2;                                            // the sorting network's size: the power of two that holds M keys
    while (P < M) P <<= 1;
    hipLaunchKernelGGL(k_pair_orderings, dim3(2), dim3(kOrdThreads), 0, S(stream), pair_drug, pair_second, real_pairs, rowptr_drug, perm_drug,
                       rowptr_second, perm_second, (int)M, (int)U, (int)Cn, P);
    return launch_status(who);
}

int64_t fn_cdrp_pair_factored_ws(int64_t U, int64_t C) { return factored_ws(U, C); }
int64_t fn_dta_pair_factored_ws(int64_t U, int64_t C) { return factored_ws(U, C); }

int fn_cdrp_pair_factored_fwd_f32(const float* drug, const float* cell, const int64_t* pair_drug, const int64_t* pair_cell, const float* W1,
                                  const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                  float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc, int64_t H,
                                  int64_t C, fn_stream_t stream) {
    return pairf_fwd<256>("fn_cdrp_pair_factored_fwd_f32", drug, cell, pair_drug, pair_cell, W1, b1, w2, b2, target, A, B, ws, out, g, loss_part,
                          M, U, Cn, Kd, Kc, H, C, nullptr, stream);
}
int fn_cdrp_pair_factored_fwd_rows_f32(const float* drug, const float* cell, const int64_t* pair_drug, const int64_t* pair_cell, const float* W1,
                                       const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                       float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc,
                                       int64_t H, int64_t C, const int32_t* real_pairs, fn_stream_t stream) {
    return pairf_fwd<256>("fn_cdrp_pair_factored_fwd_rows_f32", drug, cell, pair_drug, pair_cell, W1, b1, w2, b2, target, A, B, ws, out, g,
                          loss_part, M, U, Cn, Kd, Kc, H, C, real_pairs, stream);
}
int fn_dta_pair_factored_fwd_f32(const float* drug, const float* xt, const int64_t* pair_drug, const int64_t* pair_prot, const float* W1,
                                 const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                 float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx, int64_t H,
                                 int64_t C, fn_stream_t stream) {
    return pairf_fwd<300>("fn_dta_pair_factored_fwd_f32", drug, xt, pair_drug, pair_prot, W1, b1, w2, b2, target, A, B, ws, out, g, loss_part, M,
                          U, Cn, Kd, Kx, H, C, nullptr, stream);
}
int fn_dta_pair_factored_fwd_rows_f32(const float* drug, const float* xt, const int64_t* pair_drug, const int64_t* pair_prot, const float* W1,
                                      const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                      float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx,
                                      int64_t H, int64_t C, const int32_t* real_pairs, fn_stream_t stream) {
    return pairf_fwd<300>("fn_dta_pair_factored_fwd_rows_f32", drug, xt, pair_drug, pair_prot, W1, b1, w2, b2, target, A, B, ws, out, g,
                          loss_part, M, U, Cn, Kd, Kx, H, C, real_pairs, stream);
}

int fn_cdrp_pair_factored_bwd_f32(const float* g, const float* drug, const float* cell, const float* A, const float* B, const float* W1,
                                  const float* b1, const float* w2, const int32_t* rowptr_drug, const int32_t* perm_drug,
                                  const int32_t* rowptr_cell, const int32_t* perm_cell, float* g_drug, float* g_cell, float* dW1, float* db1,
                                  float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss, int64_t M, int64_t U, int64_t Cn,
                                  int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream) {
    return pairf_bwd<256, true>("fn_cdrp_pair_factored_bwd_f32", g, drug, cell, A, B, W1, b1, w2, rowptr_drug, perm_drug, rowptr_cell, perm_cell,
                                g_drug, g_cell, dW1, db1, dW2, db2, loss_part, n_part, loss, M, U, Cn, Kd, Kc, H, C, stream);
}
int fn_dta_pair_factored_bwd_f32(const float* g, const float* drug, const float* xt, const float* A, const float* B, const float* W1,
                                 const float* b1, const float* w2, const int32_t* rowptr_drug, const int32_t* perm_drug,
                                 const int32_t* rowptr_prot, const int32_t* perm_prot, float* g_drug, float* g_xt, float* dW1, float* db1,
                                 float* dW2, float* db2, const float* loss_part, int64_t n_part, float* loss, int64_t M, int64_t U, int64_t Cn,
                                 int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream) {
    return pairf_bwd<300, false>("fn_dta_pair_factored_bwd_f32", g, drug, xt, A, B, W1, b1, w2, rowptr_drug, perm_drug, rowptr_prot, perm_prot,
                                 g_drug, g_xt, dW1, db1, dW2, db2, loss_part, n_part, loss, M, U, Cn, Kd, Kx, H, C, stream);
}

int fn_cdrp_pair_factored_grid_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                                   float* out, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream) {
    return pairf_grid<256>("fn_cdrp_pair_factored_grid_f32", drug, cell, W1, b1, w2, b2, out, U, Cn, Kd, Kc, H, C, stream);
}
int fn_dta_pair_factored_grid_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                                  float* out, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream) {
    return pairf_grid<300>("fn_dta_pair_factored_grid_f32", drug, xt, W1, b1, w2, b2, out, U, Cn, Kd, Kx, H, C, stream);
}
}  // extern "C"
