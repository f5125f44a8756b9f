// topk.hip -- brute-force nearest neighbours in embedding space: the similarity tile and the top-k selection in one kernel, so the
// [n_q, n_lib] score matrix never exists, and a second, small kernel that folds the candidates into the caller's running lists.
// A translation unit of its own: nothing shared with the encoder's kernels but the error string.
//
// fn_topk_update_f32 folds one library chunk into running best lists [n_q, k].  Two launches, no atomics, no workgroup waits on another:
//   k_topk_scan   grid = query tiles (32 queries) x library slices; 4 waves per workgroup.  A wave keeps its two 16-query A operand
//                 sets in registers for the whole launch and walks the 16-row library tiles of its slice (tile = slice start + wave,
//                 stride 4).  Per tile: d/4 fp32-input MFMAs (16x16x4) per query set into one accumulator each, then the epilogue of
//                 the metric, then a filter against the query's threshold (the better of the incoming list's k-th entry and the
//                 wave's own k-th), and -- rarely -- a cooperative sorted insertion into the wave's own list of that query in LDS.
//                 At the end every wave writes its lists [32 queries][k] to scratch.  Waves share nothing, so there is no barrier.
//   k_topk_merge  one wave per query: a k-round selection over the heads of the incoming list and the 4 x slices scratch lists
//                 (each sorted, pairwise disjoint), winners held in registers and written back at the end.
// The score of a pair is one chain over d whatever tile, slice or chunk the library row lands in: the MFMA is bit for bit
// fma(a_k3 b_k3, fma(a_k2 b_k2, ..C)) over its four k, and the kernel feeds it k = 16 t + 4 h + c for h = 0..3 at step (t, c), t outer, c
// inner -- a fixed permutation of 0..d-1 that lets a lane fetch its operands as one float4 per 16 columns.  Every list is the exact
// top-k of its candidates under the TOTAL order (better score first, smaller global index first; the index compares unsigned, so an
// empty slot, index -1, loses to every row), the filter only drops candidates a final list cannot hold, and the top-k of a union under
// a total order does not depend on how the union was cut: results are bit-identical for every chunking and every slice count.
// Internally every score is a KEY where larger is better (squared L2 is negated: exact); lists in scratch hold keys.
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 4;             // per workgroup; each walks its own library tiles
constexpr int kQTile = 32;            // queries per workgroup: two MFMA row sets per wave
constexpr int kLTile = 16;            // library rows per MFMA
constexpr int kMaxK = 32;
constexpr int kMaxSlices = 63;        // 1 + 4 * 63 lists <= 4 per lane of the merging wave
constexpr int kMergeLists = 4;        // lists per lane in k_topk_merge

__device__ __forceinline__ bool better(float ak, uint64_t ai, float bk, uint64_t bi) { return ak > bk || (ak == bk && ai < bi); }

struct ScanArgs {
    const float *q, *lib, *q_aux, *lib_aux;
    const int64_t* exclude;
    const float* best_score;
    const int64_t* best_index;
    float* sc_key;                    // [n_q][lists][k]
    int64_t* sc_idx;
    int64_t n_q, n_lib, index_base;
    int64_t q_tiles, tiles_per_slice, n_tiles;
    int k, metric, lists;
};

template <int D>
__global__ __launch_bounds__(256) void k_topk_scan(const ScanArgs a) {
    constexpr int T = D / 16;                                     // float4 operand fetches per row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = a.k;
    // per-wave LDS: list keys [32][k], list indices [32][k], threshold key / index [32], incoming k-th key / index [32]
    uint64_t* const li = reinterpret_cast<uint64_t*>(smem) + (size_t)wave * (kQTile * k + 2 * kQTile);
    uint64_t* const thr_i = li + kQTile * k;
    uint64_t* const in_i = thr_i + kQTile;
    float* const lk = reinterpret_cast<float*>(smem + (size_t)kWaves * (kQTile * k + 2 * kQTile) * 8) + (size_t)wave * (kQTile * k + 2 * kQTile);
    float* const thr_k = lk + kQTile * k;
    float* const in_k = thr_k + kQTile;

    const int64_t qt = blockIdx.x % a.q_tiles, slice = blockIdx.x / a.q_tiles;
    const int64_t q0 = qt * kQTile;
    const float sign = a.metric == 2 ? -1.f : 1.f;
    for (int e = lane; e < kQTile * k; e += 64) { lk[e] = -INFINITY; li[e] = ~0ull; }
    if (lane < kQTile) {
        const int64_t qi = q0 + lane;
        float tk = INFINITY;                                       // rows past n_q: nothing beats the threshold
        uint64_t ti = 0;
        if (qi < a.n_q) {
            tk = sign * a.best_score[qi * k + (k - 1)];
            ti = (uint64_t)a.best_index[qi * k + (k - 1)];
        }
        thr_k[lane] = in_k[lane] = tk;
        thr_i[lane] = in_i[lane] = ti;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    const int r = lane & 15, h = lane >> 4;
    // A operands: query rows q0 + r and q0 + 16 + r (clamped: rows past n_q are computed and never become candidates)
    f32x4 qa[2][T];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        int64_t qi = q0 + 16 * s + r;
        qi = qi < a.n_q ? qi : a.n_q - 1;
        const f32x4* row = reinterpret_cast<const f32x4*>(a.q + qi * D) + h;
#pragma unroll
        for (int t = 0; t < T; ++t) qa[s][t] = row[4 * t];
    }
    // per-lane epilogue terms of its 8 query rows (set s, rows 4 h + g), and their exclusions
    float qx[2][4];
    int64_t qex[2][4];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t qi = q0 + 16 * s + 4 * h + g;
            const bool in = qi < a.n_q;
            qx[s][g] = (a.metric != 0 && in) ? a.q_aux[qi] : 0.f;
            qex[s][g] = (a.exclude && in) ? a.exclude[qi] : -1;
        }

    const int64_t t_begin = slice * a.tiles_per_slice;
    const int64_t t_end = t_begin + a.tiles_per_slice < a.n_tiles ? t_begin + a.tiles_per_slice : a.n_tiles;
    // B operands of a tile: library row tile * 16 + r, clamped to the last row -- never reads past lib + n_lib * d, whatever the tile
    auto fetch = [&](int64_t tile, f32x4* b) {
        const int64_t j = tile * kLTile + r;
        const f32x4* row = reinterpret_cast<const f32x4*>(a.lib + (j < a.n_lib ? j : a.n_lib - 1) * D) + h;
#pragma unroll
        for (int t = 0; t < T; ++t) b[t] = row[4 * t];
    };
    // d = 128: the next tile's operands are fetched under this tile's products (two waves per SIMD either way).  d = 256: the second
    // buffer would take the kernel from two waves per SIMD to one, which measured slower (4.85 -> 5.29 ms on the 512 x 1 M search).
    constexpr bool kAhead = D <= 128;
    f32x4 b[T], b_next[kAhead ? T : 1];
    if constexpr (kAhead) fetch(t_begin + wave, b);
    for (int64_t tile = t_begin + wave; tile < t_end; tile += kWaves) {
        if constexpr (kAhead) fetch(tile + kWaves, b_next);       // (past the slice: the clamped row, unused)
        else fetch(tile, b);
        const int64_t j = tile * kLTile + r;                      // this lane's library row: the B column, and the C column
        const int64_t jc = j < a.n_lib ? j : a.n_lib - 1;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[0][t][c], b[t][c], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[1][t][c], b[t][c], acc1, 0, 0, 0);
            }
        const float lx = (a.metric != 0) ? a.lib_aux[jc] : 0.f;
        const int64_t gj = a.index_base + j;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float dot = s == 0 ? acc0[g] : acc1[g];
                float key = dot;
                if (a.metric == 1) key = dot * (qx[s][g] * lx);
                else if (a.metric == 2) key = -__builtin_fmaf(-2.0f, dot, qx[s][g] + lx);
                const int ql = 16 * s + 4 * h + g;
                bool pass = j < a.n_lib && gj != qex[s][g] && key >= thr_k[ql];
                if (pass) pass = better(key, (uint64_t)gj, thr_k[ql], thr_i[ql]);
                unsigned long long mask = __ballot(pass);
                while (mask) {                                     // wave-uniform: one candidate at a time, in lane order
                    const int src = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    const float ck = __shfl(key, src);
                    const uint64_t ci = (uint64_t)(a.index_base + tile * kLTile + (src & 15));
                    const int cq = 16 * s + 4 * (src >> 4) + g;
                    if (!better(ck, ci, thr_k[cq], thr_i[cq])) continue;      // an insertion of this loop moved the threshold
                    float* const qk = lk + cq * k;
                    uint64_t* const qi = li + cq * k;
                    const bool valid = lane < k;
                    const float ek = valid ? qk[lane] : 0.f;
                    const uint64_t ei = valid ? qi[lane] : 0;
                    const bool before = valid && better(ek, ei, ck, ci);
                    const int pos = __popcll(__ballot(before));     // the list is sorted: `before` is a prefix
                    if (valid && !before && lane + 1 < k) { qk[lane + 1] = ek; qi[lane + 1] = ei; }
                    if (lane == pos) { qk[lane] = ck; qi[lane] = ci; }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    if (lane == 0) {
                        const float nk = qk[k - 1];
                        const uint64_t ni = qi[k - 1];
                        const bool own = better(nk, ni, in_k[cq], in_i[cq]);
                        thr_k[cq] = own ? nk : in_k[cq];
                        thr_i[cq] = own ? ni : in_i[cq];
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        if constexpr (kAhead) {
#pragma unroll
            for (int t = 0; t < T; ++t) b[t] = b_next[t];
        }
    }
    // the wave's lists to scratch: list number = 4 slice + wave of query q0 + ql
    const int64_t list = slice * kWaves + wave;
    for (int e = lane; e < kQTile * k; e += 64) {
        const int64_t qi = q0 + e / k;
        if (qi < a.n_q) {
            const int64_t o = (qi * a.lists + list) * k + e % k;
            a.sc_key[o] = lk[e];
            a.sc_idx[o] = (int64_t)li[e];
        }
    }
}

// one wave per query, 4 queries per workgroup: list 0 is the incoming list (scores -> keys), lists 1.. are the scratch lists
__global__ __launch_bounds__(256) void k_topk_merge(const float* __restrict__ sc_key, const int64_t* __restrict__ sc_idx, float* best_score,
                                                    int64_t* best_index, int64_t n_q, int k, int lists, int metric) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_q) return;
    const float sign = metric == 2 ? -1.f : 1.f;
    const int total = lists + 1;
    int ptr[kMergeLists];
    float hk[kMergeLists];
    uint64_t hi[kMergeLists];
    auto head = [&](int m) {
        const int l = lane + 64 * m;
        hk[m] = -INFINITY;
        hi[m] = ~0ull;
        if (l < total && ptr[m] < k) {
            if (l == 0) {
                hk[m] = sign * best_score[q * k + ptr[m]];
                hi[m] = (uint64_t)best_index[q * k + ptr[m]];
            } else {
                const int64_t o = (q * lists + (l - 1)) * k + ptr[m];
                hk[m] = sc_key[o];
                hi[m] = (uint64_t)sc_idx[o];
            }
        }
    };
#pragma unroll
    for (int m = 0; m < kMergeLists; ++m) { ptr[m] = 0; head(m); }
    float out_k = -INFINITY;
    uint64_t out_i = ~0ull;
    for (int round = 0; round < k; ++round) {
        float bk = hk[0];
        uint64_t bi = hi[0];
        int bm = 0;
#pragma unroll
        for (int m = 1; m < kMergeLists; ++m)
            if (better(hk[m], hi[m], bk, bi)) { bk = hk[m]; bi = hi[m]; bm = m; }
        float wk = bk;
        uint64_t wi = bi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ok = __shfl_xor(wk, off);
            const uint64_t oi = (uint64_t)__shfl_xor((long long)wi, off);
            if (better(ok, oi, wk, wi)) { wk = ok; wi = oi; }
        }
        if (wi == ~0ull) break;                                    // only empty slots are left: the rest of the list stays empty
        if (lane == round) { out_k = wk; out_i = wi; }
        if (wk == bk && wi == bi) {                                // the winner's lane (indices are distinct): advance that list
#pragma unroll
            for (int m = 0; m < kMergeLists; ++m)
                if (m == bm) { ++ptr[m]; head(m); }
        }
    }
    // every head was read before this point by this wave alone; the incoming list may now be overwritten
    if (lane < k) {
        best_score[q * k + lane] = out_i == ~0ull ? sign * -INFINITY : sign * out_k;
        best_index[q * k + lane] = (int64_t)out_i;
    }
}

// out[i] = 1 / max(|x_i|, 1e-12): one wave per row, lane l sums columns l, l + 64, .. in order, then a fixed xor butterfly
__global__ __launch_bounds__(256) void k_rows_rnorm(const float* __restrict__ x, int64_t n, int64_t d, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {
        const float* p = x + row * d;
        float s = 0.f;
        for (int64_t c = lane; c < d; c += 64) s = __builtin_fmaf(p[c], p[c], s);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) out[row] = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    }
}

struct Geometry { int64_t q_tiles, n_tiles, tiles_per_slice; int slices; };

// the launch shape is a function of the sizes alone (and of t->splits when given); the result does not depend on it
bool geometry(const fn_topk* t, Geometry* g) {
    if (!t || t->n_q < 0 || t->n_lib < 0 || t->k < 1 || t->k > kMaxK || t->splits < 0 || t->n_lib >= (1ll << 40) || t->n_q >= (1ll << 40))
        return false;
    g->q_tiles = (t->n_q + kQTile - 1) / kQTile;
    g->n_tiles = (t->n_lib + kLTile - 1) / kLTile;
    int64_t s = t->splits;
    if (s == 0) {                                                  // enough workgroups for the device, at least 2 tiles a wave
        const int64_t want = g->q_tiles > 0 ? (1024 + g->q_tiles - 1) / g->q_tiles : 1;
        const int64_t fit = (g->n_tiles + 2 * kWaves - 1) / (2 * kWaves);
        s = want < fit ? want : fit;
    }
    s = s < 1 ? 1 : s > kMaxSlices ? kMaxSlices : s;
    if (g->n_tiles > 0 && s > g->n_tiles) s = g->n_tiles;
    g->tiles_per_slice = g->n_tiles > 0 ? (g->n_tiles + s - 1) / s : 0;
    g->slices = g->n_tiles > 0 ? (int)((g->n_tiles + g->tiles_per_slice - 1) / g->tiles_per_slice) : 1;
    return true;
}

int64_t scratch_bytes(const fn_topk* t, const Geometry& g) { return t->n_q * (int64_t)g.slices * kWaves * t->k * 12; }

}  // namespace

extern "C" {

int fn_rows_rnorm_f32(const float* x, int64_t n, int64_t d, float* out, fn_stream_t stream) {
    if (n < 0 || d < 0) return fail(FN_EINVAL, "fn_rows_rnorm_f32: negative size");
    if (n == 0) return 0;
    if (!x || !out || (((uintptr_t)x | (uintptr_t)out) & 3)) return fail(FN_EINVAL, "fn_rows_rnorm_f32: null or misaligned buffer");
    const int64_t blocks = (n + 3) / 4;
    hipLaunchKernelGGL(k_rows_rnorm, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, S(stream), x, n, d, out);
    return launch_status("fn_rows_rnorm_f32");
}

int64_t fn_topk_scratch_bytes(const fn_topk* t) {
    Geometry g;
    if (!geometry(t, &g)) return fail(FN_EINVAL, "fn_topk_scratch_bytes: null descriptor, negative size, or k outside [1, 32]");
    return scratch_bytes(t, g);
}

int fn_topk_update_f32(const fn_topk* t, fn_stream_t stream) {
    Geometry g;
    if (!geometry(t, &g)) return fail(FN_EINVAL, "fn_topk_update_f32: null descriptor, negative size, or k outside [1, 32]");
    if (t->metric < 0 || t->metric > 2) return fail(FN_EINVAL, "fn_topk_update_f32: metric is 0 (dot), 1 (cosine) or 2 (squared L2)");
    if (t->d != 128 && t->d != 256) return fail(FN_EUNSUPPORTED, "fn_topk_update_f32: rows are 128 or 256 floats wide");
    if (t->n_q == 0 || t->n_lib == 0) return 0;
    if (!t->q || !t->lib || !t->best_score || !t->best_index || !t->scratch || (t->metric != 0 && (!t->q_aux || !t->lib_aux)))
        return fail(FN_EINVAL, "fn_topk_update_f32: null buffer (q, lib, the lists, scratch; q_aux and lib_aux unless metric is 0)");
    if ((((uintptr_t)t->q | (uintptr_t)t->lib | (uintptr_t)t->scratch) & 15) || (((uintptr_t)t->best_index | (uintptr_t)t->exclude) & 7) ||
        (((uintptr_t)t->best_score | (uintptr_t)t->q_aux | (uintptr_t)t->lib_aux) & 3))
        return fail(FN_EINVAL, "fn_topk_update_f32: misaligned buffer (q, lib, scratch: 16 bytes; int64: 8; float: 4)");
    if (t->scratch_bytes < scratch_bytes(t, g)) return fail(FN_EINVAL, "fn_topk_update_f32: scratch smaller than fn_topk_scratch_bytes");
    if (g.q_tiles * g.slices >= (1ll << 31)) return fail(FN_EINVAL, "fn_topk_update_f32: more than 2^31 workgroups; fold fewer queries per call");

    ScanArgs a;
    a.q = t->q; a.lib = t->lib; a.q_aux = t->q_aux; a.lib_aux = t->lib_aux; a.exclude = t->exclude;
    a.best_score = t->best_score; a.best_index = t->best_index;
    a.lists = g.slices * kWaves;
    a.sc_idx = reinterpret_cast<int64_t*>(t->scratch);              // the int64 half first: both halves stay aligned
    a.sc_key = reinterpret_cast<float*>(a.sc_idx + t->n_q * a.lists * t->k);
    a.n_q = t->n_q; a.n_lib = t->n_lib; a.index_base = t->index_base;
    a.q_tiles = g.q_tiles; a.tiles_per_slice = g.tiles_per_slice; a.n_tiles = g.n_tiles;
    a.k = t->k; a.metric = t->metric;
    const size_t lds = (size_t)kWaves * (kQTile * t->k + 2 * kQTile) * 12;   // <= 54 KB
    const dim3 grid((unsigned)(g.q_tiles * g.slices));
    if (t->d == 128) hipLaunchKernelGGL(k_topk_scan<128>, grid, dim3(256), lds, S(stream), a);
    else hipLaunchKernelGGL(k_topk_scan<256>, grid, dim3(256), lds, S(stream), a);
    FN_TRY(launch_status("fn_topk_update_f32 (scan)"));
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)((t->n_q + 3) / 4)), dim3(256), 0, S(stream), a.sc_key, a.sc_idx, t->best_score,
                       t->best_index, t->n_q, t->k, a.lists, t->metric);
    return launch_status("fn_topk_update_f32 (merge)");
}

}  // extern "C"
