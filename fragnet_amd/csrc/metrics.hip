// metrics.hip -- evaluation metrics on the device: exact ordered-pair concordance counts (ROC-AUC on binary labels, the concordance
// index on real ones) and the fp64 sums behind MSE / MAE / Pearson / R^2.  A translation unit of its own: nothing shared with the
// encoder's kernels but the error string.
//
// fn_pair_concordance_f32: two launches, no atomics, no memset.
//   k_conc_count    grid = (i-blocks, j-slices, columns), 128 threads.  A workgroup takes i-tiles of kTile rows (its own, then every
//                   gridDim.x-th) against the j-tiles of its slice.  A lane keeps kLaneRows i-rows (pred, label) in registers; the j-tile is
//                   staged once in LDS as (pred, label) pairs and walked with 16-byte reads of the SAME address in every lane -- a
//                   broadcast, conflict-free -- so one LDS read feeds 2 x kLaneRows pair updates.  A pair update is three compares and three
//                   add-with-carry on 32-bit lane counters (at most kLaneRows * 2^24 per i-tile), widened to 64 bits per i-tile.
//                   Validity costs the inner loop nothing: an i-row that is invalid (label below the floor, NaN label, NaN prediction,
//                   past n) is given the label -inf and a j-row the label +inf, and `label_i > label_j` is then false for every
//                   partner.  (A VALID -inf as i or +inf as j takes part in no pair either: nothing is below -inf or above +inf.)
//                   The workgroup's five sums go to its own row of scratch; n_valid and n_nan are counted by slice 0 alone.
//   k_conc_combine  one workgroup per column adds that column's rows.  Integer sums: any order gives the same bits.
// fn_regression_sums_f32: the same two steps over chunks of kChunk rows, in fp64 and in one fixed order (header comment).
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

constexpr int kTile = FN_CONC_TILE;       // rows of an i-tile and of a j-tile
constexpr int kThreads = 128;             // k_conc_count
constexpr int kLaneRows = kTile / kThreads;   // i-rows per lane
constexpr int kMaxIBlocks = 4096;         // i-tiles beyond this are walked by the same workgroups
constexpr int kMaxSlices = 1024;
constexpr int kWantBlocks = 2048;         // 256 CUs x 8 workgroups of two waves
constexpr int kChunk = FN_SUMS_CHUNK;
constexpr int kSumThreads = 256;
constexpr int64_t kMaxN = 1ll << 24;
static_assert(kLaneRows == 4 && kTile % 2 == 0, "a lane keeps four i-rows; the j-tile is read two rows at a time");
static_assert(kChunk % kSumThreads == 0, "a chunk is whole passes of the workgroup");

struct ConcArgs {
    const float *pred, *label;
    unsigned long long* part;             // [c][slices][i_blocks][FN_CONC_FIELDS]
    int64_t n;
    float floor;
    int c, i_tiles, j_tiles, tiles_per_slice;
};

// sum over the workgroup of F 64-bit values per thread; the result is valid in thread 0
template <int F, int WAVES, typename T> __device__ __forceinline__ void block_sum(T (&v)[F], T* lds /*[WAVES][F]*/) {
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[f] += __shfl_xor(v[f], off);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                               // lds may still be read from the previous use
    if (lane == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) lds[wave * F + f] = v[f];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) {
            T t = lds[f];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) t += lds[w * F + f];   // the wave sums in order
            v[f] = t;
        }
}

__global__ __launch_bounds__(kThreads) void k_conc_count(const ConcArgs a) {
    __shared__ float4 tile[kTile / 2];                             // (pred_j, label_j, pred_j+1, label_j+1)
    __shared__ unsigned long long red[(kThreads / 64) * FN_CONC_FIELDS];
    const int tid = threadIdx.x, col = blockIdx.z, slice = blockIdx.y, c = a.c;
    const int jt0 = slice * a.tiles_per_slice;
    const int jt1 = jt0 + a.tiles_per_slice < a.j_tiles ? jt0 + a.tiles_per_slice : a.j_tiles;
    // n_valid, n_nan, n_pairs, n_conc, n_tied of this lane
    unsigned long long sum[FN_CONC_FIELDS] = {0, 0, 0, 0, 0};
    for (int it = blockIdx.x; it < a.i_tiles; it += gridDim.x) {
        float pi[kLaneRows], li[kLaneRows];
#pragma unroll
        for (int r = 0; r < kLaneRows; ++r) {
            const int64_t i = (int64_t)it * kTile + r * kThreads + tid;
            float p = 0.f, l = -INFINITY;
            bool valid = false;
            if (i < a.n) {
                p = a.pred[i * c + col];
                l = a.label[i * c + col];
                valid = l >= a.floor;                              // false for a NaN label
            }
            const bool nan = valid && p != p;
            if (slice == 0) { sum[0] += valid; sum[1] += nan; }
            const bool ok = valid && !nan;
            li[r] = ok ? l : -INFINITY;
            pi[r] = ok ? p : 0.f;
        }
        unsigned pairs = 0, conc = 0, tied = 0;
        for (int jt = jt0; jt < jt1; ++jt) {
            __syncthreads();                                       // the previous tile has been walked by every wave
            float* const flat = reinterpret_cast<float*>(tile);
#pragma unroll
            for (int k = 0; k < kLaneRows; ++k) {
                const int e = k * kThreads + tid;
                const int64_t j = (int64_t)jt * kTile + e;
                float p = 0.f, l = INFINITY;
                if (j < a.n) {
                    const float pj = a.pred[j * c + col], lj = a.label[j * c + col];
                    if (lj >= a.floor && pj == pj) { p = pj; l = lj; }
                }
                flat[2 * e] = p;
                flat[2 * e + 1] = l;
            }
            __syncthreads();
#pragma unroll 4
            for (int q = 0; q < kTile / 2; ++q) {
                const float4 v = tile[q];
#pragma unroll
                for (int r = 0; r < kLaneRows; ++r) {
                    const bool g0 = li[r] > v.y, g1 = li[r] > v.w;
                    pairs += g0;
                    conc += g0 & (pi[r] > v.x);
                    tied += g0 & (pi[r] == v.x);
                    pairs += g1;
                    conc += g1 & (pi[r] > v.z);
                    tied += g1 & (pi[r] == v.z);
                }
            }
        }
        sum[2] += pairs; sum[3] += conc; sum[4] += tied;
    }
    block_sum<FN_CONC_FIELDS, kThreads / 64>(sum, red);
    if (tid == 0) {
        unsigned long long* row = a.part + (((size_t)col * gridDim.y + slice) * gridDim.x + blockIdx.x) * FN_CONC_FIELDS;
#pragma unroll
        for (int f = 0; f < FN_CONC_FIELDS; ++f) row[f] = sum[f];
    }
}

__global__ __launch_bounds__(kSumThreads) void k_conc_combine(const unsigned long long* __restrict__ part, int64_t rows,
                                                              unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[(kSumThreads / 64) * FN_CONC_FIELDS];
    const unsigned long long* p = part + (size_t)blockIdx.x * rows * FN_CONC_FIELDS;
    unsigned long long sum[FN_CONC_FIELDS] = {0, 0, 0, 0, 0};
    for (int64_t r = threadIdx.x; r < rows; r += kSumThreads)
#pragma unroll
        for (int f = 0; f < FN_CONC_FIELDS; ++f) sum[f] += p[r * FN_CONC_FIELDS + f];
    block_sum<FN_CONC_FIELDS, kSumThreads / 64>(sum, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < FN_CONC_FIELDS; ++f) out[(size_t)blockIdx.x * FN_CONC_FIELDS + f] = sum[f];
}

// pred * scale + shift as numpy evaluates it on float32: a rounded product, then a rounded sum -- never one fma
__device__ __forceinline__ float scale_shift(float p, float scale, float shift) {
#pragma clang fp contract(off)
    const float m = p * scale;
    return m + shift;
}

// one row of FN_SUMS_FIELDS doubles per (column, chunk): part [c][n_chunks][FN_SUMS_FIELDS]
__global__ __launch_bounds__(kSumThreads) void k_sums_chunks(const float* __restrict__ pred, const float* __restrict__ label, int64_t n, int c,
                                                             float floor, float scale, float shift, int64_t n_chunks, double* __restrict__ part) {
    __shared__ double red[(kSumThreads / 64) * FN_SUMS_FIELDS];
    const int col = blockIdx.y;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        double s[FN_SUMS_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < kChunk / kSumThreads; ++k) {
            const int64_t i = chunk * kChunk + k * kSumThreads + threadIdx.x;
            if (i >= n) continue;
            const float l = label[i * c + col];
            if (!(l >= floor)) continue;
            const double y = l, p = scale_shift(pred[i * c + col], scale, shift), d = y - p;
            s[0] += 1.0; s[1] += y; s[2] += p; s[3] += y * y; s[4] += p * p; s[5] += y * p; s[6] += d * d; s[7] += fabs(d);
        }
        block_sum<FN_SUMS_FIELDS, kSumThreads / 64>(s, red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int f = 0; f < FN_SUMS_FIELDS; ++f) part[((size_t)col * n_chunks + chunk) * FN_SUMS_FIELDS + f] = s[f];
    }
}

__global__ __launch_bounds__(kSumThreads) void k_sums_combine(const double* __restrict__ part, int64_t n_chunks, double* __restrict__ out) {
    __shared__ double red[(kSumThreads / 64) * FN_SUMS_FIELDS];
    const double* p = part + (size_t)blockIdx.x * n_chunks * FN_SUMS_FIELDS;
    double s[FN_SUMS_FIELDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int64_t r = threadIdx.x; r < n_chunks; r += kSumThreads)
#pragma unroll
        for (int f = 0; f < FN_SUMS_FIELDS; ++f) s[f] += p[r * FN_SUMS_FIELDS + f];
    block_sum<FN_SUMS_FIELDS, kSumThreads / 64>(s, red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < FN_SUMS_FIELDS; ++f) out[(size_t)blockIdx.x * FN_SUMS_FIELDS + f] = s[f];
}

struct Geometry {
    int i_tiles, j_tiles, i_blocks, tiles_per_slice, slices;       // concordance
    int64_t n_chunks;                                              // sums
    int sum_blocks;
};

// the launch shape is a function of n, c and splits alone; no result depends on it
bool geometry(const fn_metrics* m, Geometry* g) {
    if (!m || m->n < 0 || m->n > kMaxN || m->c < 1 || m->c > FN_METRICS_MAX_COLS || m->splits < 0) return false;
    const int tiles = (int)((m->n + kTile - 1) / kTile);
    g->i_tiles = g->j_tiles = tiles;
    g->i_blocks = tiles < kMaxIBlocks ? tiles : kMaxIBlocks;
    int s = m->splits;
    if (s == 0) s = g->i_blocks > 0 ? (kWantBlocks + g->i_blocks * m->c - 1) / (g->i_blocks * m->c) : 1;
    s = s > kMaxSlices ? kMaxSlices : s;
    s = s > tiles ? tiles : s;
    s = s < 1 ? 1 : s;
    g->tiles_per_slice = tiles > 0 ? (tiles + s - 1) / s : 0;
    g->slices = tiles > 0 ? (tiles + g->tiles_per_slice - 1) / g->tiles_per_slice : 1;
    g->n_chunks = (m->n + kChunk - 1) / kChunk;
    int64_t b = m->splits ? m->splits : g->n_chunks;
    b = b > g->n_chunks ? g->n_chunks : b;
    b = b > 65535 ? 65535 : b;
    g->sum_blocks = (int)(b < 1 ? 1 : b);
    return true;
}

int64_t scratch_bytes(const fn_metrics* m, const Geometry& g, bool sums) {
    return sums ? (int64_t)m->c * g.n_chunks * FN_SUMS_FIELDS * 8 : (int64_t)m->c * g.slices * g.i_blocks * FN_CONC_FIELDS * 8;
}

// what both launchers check before anything touches the GPU; *g is filled
int check(const fn_metrics* m, bool sums, Geometry* g, const char* bad_desc, const char* bad_buf, const char* bad_scratch) {
    if (!geometry(m, g)) return fail(FN_EINVAL, bad_desc);
    // (n = 0 reads no row: an empty tensor's pointers may be null)
    if (!m->out || (m->n > 0 && (!m->pred || !m->label)) || misaligned(3, m->pred, m->label) || misaligned(7, m->out, m->scratch)) return fail(FN_EINVAL, bad_buf);
    if (m->n > 0 && (!m->scratch || m->scratch_bytes < scratch_bytes(m, *g, sums))) return fail(FN_EINVAL, bad_scratch);
    return 0;
}

}  // namespace

extern "C" {

int64_t fn_metrics_scratch_bytes(const fn_metrics* m, int sums) {
    Geometry g;
    if (!geometry(m, &g)) return fail(FN_EINVAL, "fn_metrics_scratch_bytes: null descriptor, n outside [0, 2^24], c outside [1, 64] or negative splits");
    return scratch_bytes(m, g, sums != 0);
}

int fn_pair_concordance_f32(const fn_metrics* m, fn_stream_t stream) {
    Geometry g;
    FN_TRY(check(m, false, &g, "fn_pair_concordance_f32: null descriptor, n outside [0, 2^24], c outside [1, 64] or negative splits",
                 "fn_pair_concordance_f32: null or misaligned buffer (pred, label: 4 bytes; out, scratch: 8)",
                 "fn_pair_concordance_f32: scratch is null or smaller than fn_metrics_scratch_bytes(m, 0)"));
    unsigned long long* out = reinterpret_cast<unsigned long long*>(m->out);
    if (m->n == 0) {
        if (hipMemsetAsync(out, 0, (size_t)m->c * FN_CONC_FIELDS * 8, S(stream)) != hipSuccess) return launch_status("fn_pair_concordance_f32 (zeros)");
        return 0;
    }
    ConcArgs a;
    a.pred = m->pred; a.label = m->label; a.part = reinterpret_cast<unsigned long long*>(m->scratch);
    a.n = m->n; a.floor = m->label_floor; a.c = m->c;
    a.i_tiles = g.i_tiles; a.j_tiles = g.j_tiles; a.tiles_per_slice = g.tiles_per_slice;
    hipLaunchKernelGGL(k_conc_count, dim3((unsigned)g.i_blocks, (unsigned)g.slices, (unsigned)m->c), dim3(kThreads), 0, S(stream), a);
    FN_TRY(launch_status("fn_pair_concordance_f32 (count)"));
    hipLaunchKernelGGL(k_conc_combine, dim3((unsigned)m->c), dim3(kSumThreads), 0, S(stream), a.part, (int64_t)g.slices * g.i_blocks, out);
    return launch_status("fn_pair_concordance_f32 (combine)");
}

int fn_regression_sums_f32(const fn_metrics* m, fn_stream_t stream) {
    Geometry g;
    FN_TRY(check(m, true, &g, "fn_regression_sums_f32: null descriptor, n outside [0, 2^24], c outside [1, 64] or negative splits",
                 "fn_regression_sums_f32: null or misaligned buffer (pred, label: 4 bytes; out, scratch: 8)",
                 "fn_regression_sums_f32: scratch is null or smaller than fn_metrics_scratch_bytes(m, 1)"));
    double* out = reinterpret_cast<double*>(m->out);
    if (m->n == 0) {
        if (hipMemsetAsync(out, 0, (size_t)m->c * FN_SUMS_FIELDS * 8, S(stream)) != hipSuccess) return launch_status("fn_regression_sums_f32 (zeros)");
        return 0;
    }
    double* part = reinterpret_cast<double*>(m->scratch);
    hipLaunchKernelGGL(k_sums_chunks, dim3((unsigned)g.sum_blocks, (unsigned)m->c), dim3(kSumThreads), 0, S(stream), m->pred, m->label, m->n, (int)m->c,
                       m->label_floor, m->scale, m->shift, g.n_chunks, part);
    FN_TRY(launch_status("fn_regression_sums_f32 (chunks)"));
    hipLaunchKernelGGL(k_sums_combine, dim3((unsigned)m->c), dim3(kSumThreads), 0, S(stream), part, g.n_chunks, out);
    return launch_status("fn_regression_sums_f32 (combine)");
}

}  // extern "C"
