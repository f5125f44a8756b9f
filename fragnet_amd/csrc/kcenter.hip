// kcenter.hip -- greedy k-centre (Gonzalez; farthest-point / MaxMin picking) over embedding rows x [n, d]: mind[i] is the distance of
// row i to its nearest centre so far, a pick is the unpicked row with the largest mind, and folding the new centre in lowers mind.
// A translation unit of its own: nothing shared with the encoder's kernels but the error string.
//
// One launch per pick (k_kc_pass), no atomics, no workgroup waits on another, nothing synchronises with the host:
//   prologue  every workgroup reduces the previous launch's partial table -- <= 512 (key, row) pairs, one per workgroup of that launch --
//             under the TOTAL order (larger key first, on equal keys the smaller row), so every workgroup arrives at the same winner c
//             and the same ordinal t (the count travels in the table's header).  Workgroup 0 alone records picked[t], radius[t] and
//             the new count in the table it writes.  Every workgroup reads row c (and aux[c]) once: the same lines for all of them.
//   body      the workgroup's tiles (32 rows at d = 256, 64 at d = 128, tile = workgroup, stride grid) stream through as 16-byte loads
//             per lane, eight per lane in flight: one wave covers a row per load at d = 256, a half-wave at d = 128.  Per row: the
//             lane's four columns in order as one fma chain, then the xor butterfly 1, 2, 4, 8, 16 (, 32) -- ONE order of addition,
//             whatever n, the grid, splits, or the call a pass belongs to.  Eight lanes per (half-)wave then own a row each: the
//             strict update `dist < mind` (stored only when lowered), and a running best of the rows they own.
//   epilogue  block arg-max -> entry blockIdx.x of this launch's table.  Two tables in ping-pong: launch q reads q - 1's, writes q's.
// A pick call whose first centre is the arg-max (first = -1) opens with a SCAN launch (the body without a centre: it reads mind alone)
// and every call ends with k_kc_close, the prologue alone, which writes radius[count] and the count word.  So the count word is read
// by the first launch of a call and written by the last, never both in one launch; in between it lives in the tables.
// A picked row is marked in mind itself: its mind is stored as -0.0f (it IS at distance zero of a centre; the sign bit says "taken").
// The mark is the whole state of a run besides the caller's arrays, so pick(a) then pick(b) continues exactly where pick(a + b) would
// be: the scratch carries nothing from call to call.
// Keys: a taken row has none; a NaN mind has key -1 (below every distance, so it never wins while a number is left, and among NaNs
// the smallest row wins); else the key is mind.  NaN distances compare false and lower nothing.
//
// Supposed, not measured: that re-reducing <= 512 pairs in every workgroup (6 KB from L2) costs less than the 1.5-1.9 us of one more
// dependent launch per pick -- there is no A/B against a separate merge launch.  Measured on one MI355X (DESIGN.md 7q,
// profiles/diversity_kcenter.txt; k = 256, squared L2): 24.2 / 14.4 us per pick at 131 072 rows of 256 / 128 floats, 174.7 / 91.3 us at
// 1 M rows (6.1 / 5.9 TB/s of the rows), 5.8-6.3 x the torch route sub, square, sum, minimum, argmax on the same rows.  At 131 072 x 128
// a whole pick is 14.4 us for 64 MiB, which bounds boundary + prologue + epilogue at a few microseconds.
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

constexpr int kMaxGrid = 512;                 // workgroups per pass = entries of a partial table
constexpr int kInFlight = 8;                  // 16-byte loads per lane and step
constexpr float kNoKey = -2.f, kNaNKey = -1.f;
constexpr int64_t kNoRow = INT64_MAX;
constexpr uint32_t kTakenBits = 0x80000000u;  // -0.0f
enum { kScan = 0, kGiven = 1, kTable = 2, kSeed = 3 };

struct Table {
    int64_t count, pad;                       // centres folded in once the launch that wrote this table is done
    int64_t row[kMaxGrid];
    float key[kMaxGrid];
};
static_assert(sizeof(Table) == 16 + 12 * kMaxGrid && sizeof(Table) % 16 == 0, "two tables back to back stay 16-byte aligned");

struct Best { float key; int64_t row; };

__device__ __forceinline__ bool better(float ak, int64_t ai, float bk, int64_t bi) { return ak > bk || (ak == bk && ai < bi); }

// the same pair in every thread of the workgroup; s4 is free again on return
__device__ __forceinline__ Best block_best(Best b, Best* s4) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ok = __shfl_xor(b.key, off);
        const int64_t oi = (int64_t)__shfl_xor((long long)b.row, off);
        if (better(ok, oi, b.key, b.row)) { b.key = ok; b.row = oi; }
    }
    if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = b;
    __syncthreads();
    Best r = s4[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (better(s4[w].key, s4[w].row, r.key, r.row)) r = s4[w];
    __syncthreads();
    return r;
}

__device__ __forceinline__ Best table_best(const Table* t, int entries, Best* s4) {
    Best b = {kNoKey, kNoRow};
    for (int e = threadIdx.x; e < entries; e += 256) {
        const float k = t->key[e];
        const int64_t r = t->row[e];
        if (better(k, r, b.key, b.row)) { b.key = k; b.row = r; }
    }
    return block_best(b, s4);
}

__device__ __forceinline__ float key_value(float key) { return key == kNoKey ? 0.f : key == kNaNKey ? __builtin_nanf("") : key; }

struct PassArgs {
    const float *x, *aux;
    float* mind;
    int32_t* label;
    int64_t* picked;
    float* radius;
    const int64_t* count;                     // the count word: read by kScan / kGiven / kSeed
    const Table* prev;                        // kTable
    Table* next;                              // all but kSeed
    const float *centre, *centre_aux;         // kSeed: the centre's row and (metric 1) its reciprocal norm
    int64_t n, cap, first, seed_index;
    int mode, prev_entries;
};

template <int D, int METRIC>
__global__ __launch_bounds__(256) void k_kc_pass(const PassArgs a) {
    __shared__ Best s4[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- prologue: the centre c of this pass (none: a scan), its ordinal t
    int64_t count = a.mode == kTable ? a.prev->count : *a.count;
    int64_t c = -1;
    float ckey = 0.f;
    bool update = false;
    if (a.mode == kTable) {
        const Best w = table_best(a.prev, a.prev_entries, s4);
        if (w.key != kNoKey && count < a.cap) { c = w.row; update = true; }       // (else: no row left, or picked is full -- a scan)
        ckey = w.key;
    } else if (a.mode == kGiven) {
        if (count < a.cap) { c = a.first; update = true; }
    } else if (a.mode == kSeed) {
        count += a.seed_index;
        update = true;
    }
    const int32_t t = (int32_t)count;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.mode != kSeed) {
        if (update) {
            a.picked[t] = c;
            if (a.mode == kTable) a.radius[t] = key_value(ckey);                   // (kGiven: the lane that owns row c writes it, below)
        }
        a.next->count = count + (update ? 1 : 0);
    }
    constexpr int LPR = D / 4;                 // lanes per row
    constexpr int RPI = 64 / LPR;              // rows per load instruction of a wave
    constexpr int WROWS = kInFlight * RPI;     // rows per wave and step
    constexpr int TROWS = 4 * WROWS;           // rows per tile
    const int col = (lane & (LPR - 1)) * 4, half = lane / LPR, u = lane & 31;
    float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
    float caux = 0.f;
    if (update) {
        cv = ld4((a.mode == kSeed ? a.centre : a.x + c * D) + col);
        if (METRIC == 1) caux = a.mode == kSeed ? *a.centre_aux : a.aux[c];
    }
    // ---- body
    const bool owner = u < kInFlight && (RPI == 2 || lane < 32);                   // this lane owns row 2 u + half (d = 128) or u of the step
    Best best = {kNoKey, kNoRow};
    const int64_t tiles = (a.n + TROWS - 1) / TROWS;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t base = tile * TROWS + wave * WROWS;
        if (base >= a.n) continue;                                                 // (wave-uniform)
        const int64_t mine = base + (RPI == 2 ? 2 * u + half : u);
        const bool own = owner && mine < a.n;
        float m = 0.f, dist = 0.f;
        if (own) m = a.mind[mine];
        if (update) {
            float4 v[kInFlight];
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) {                                  // rows past n: the last row again, owned by nobody
                const int64_t r = base + j * RPI + half;
                v[j] = ld4(a.x + (r < a.n ? r : a.n - 1) * D + col);
            }
            const float raux = (METRIC == 1 && own) ? a.aux[mine] : 0.f;
#pragma unroll
            for (int j = 0; j < kInFlight; ++j) {
                float s = 0.f;
                if (METRIC == 0) {
                    const float d0 = v[j].x - cv.x, d1 = v[j].y - cv.y, d2 = v[j].z - cv.z, d3 = v[j].w - cv.w;
                    s = __builtin_fmaf(d3, d3, __builtin_fmaf(d2, d2, __builtin_fmaf(d1, d1, __builtin_fmaf(d0, d0, 0.f))));
                } else {
                    s = __builtin_fmaf(v[j].w, cv.w, __builtin_fmaf(v[j].z, cv.z, __builtin_fmaf(v[j].y, cv.y, __builtin_fmaf(v[j].x, cv.x, 0.f))));
                }
#pragma unroll
                for (int off = 1; off < LPR; off <<= 1) s += __shfl_xor(s, off);
                if (u == j) dist = s;
            }
            if (METRIC == 1) {
                const float w = 1.0f - dist * (raux * caux);
                dist = w < 0.f ? 0.f : w;                                           // (a NaN stays a NaN)
            }
        }
        if (own) {
            bool taken = __builtin_bit_cast(uint32_t, m) == kTakenBits;
            if (update) {
                if (a.mode == kGiven && mine == c) a.radius[t] = m;
                bool lowered = dist < m;
                if (lowered) { m = dist; a.label[mine] = t; }
                if (mine == c) { m = -0.0f; taken = lowered = true; }
                if (lowered) a.mind[mine] = m;
            }
            const float key = m != m ? kNaNKey : m;
            if (!taken && better(key, mine, best.key, best.row)) { best.key = key; best.row = mine; }
        }
    }
    // ---- epilogue
    if (a.mode == kSeed) return;
    best = block_best(best, s4);
    if (threadIdx.x == 0) { a.next->key[blockIdx.x] = best.key; a.next->row[blockIdx.x] = best.row; }
}

// the prologue alone: the largest remaining mind is the coverage radius of everything chosen; the count goes back to its word
__global__ __launch_bounds__(256) void k_kc_close(const Table* prev, int prev_entries, float* radius, int64_t* count, int64_t cap) {
    __shared__ Best s4[4];
    const Best w = table_best(prev, prev_entries, s4);
    if (threadIdx.x == 0) {
        const int64_t n = prev->count;
        *count = n;
        if (n <= cap) radius[n] = key_value(w.key);
    }
}

// seeds are no rows of x: picked -1, radius NaN
__global__ __launch_bounds__(256) void k_kc_seed_close(int64_t* picked, float* radius, int64_t* count, int64_t s, int64_t cap) {
    const int64_t c0 = *count;
    for (int64_t i = threadIdx.x; i < s && c0 + i < cap; i += 256) {
        picked[c0 + i] = -1;
        radius[c0 + i] = __builtin_nanf("");
    }
    __syncthreads();
    if (threadIdx.x == 0) *count = c0 + s < cap ? c0 + s : cap;
}

constexpr int64_t kScratchBytes = 2 * (int64_t)sizeof(Table);

// what both entry points check; the launch shape is a function of n, d and splits alone, and no result depends on it
int check(const fn_kcenter* k, int* grid) {
    if (!k || k->n < 0 || k->cap < 0 || k->splits < 0 || k->host_count < 0 || k->host_picks < 0 || k->n >= (1ll << 40) || k->cap >= (1ll << 31))
        return fail(FN_EINVAL, "fn_kcenter: null descriptor, negative size or count, n >= 2^40 or cap >= 2^31");
    if (k->metric < 0 || k->metric > 1) return fail(FN_EINVAL, "fn_kcenter: metric is 0 (squared L2) or 1 (cosine distance)");
    if (k->d != 128 && k->d != 256) return fail(FN_EUNSUPPORTED, "fn_kcenter: rows are 128 or 256 floats wide");
    const int64_t trows = k->d == 256 ? 4 * kInFlight : 8 * kInFlight;
    int64_t g = (k->n + trows - 1) / trows;
    if (k->splits > 0 && k->splits < g) g = k->splits;
    *grid = (int)(g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g);
    return 0;
}

int check_buffers(const fn_kcenter* k) {
    if (!k->x || !k->mind || !k->label || !k->picked || !k->radius || !k->count || !k->scratch || (k->metric == 1 && !k->aux))
        return fail(FN_EINVAL, "fn_kcenter: null buffer (x, mind, label, picked, radius, count, scratch; aux for metric 1)");
    if (misaligned(15, k->x, k->scratch) || misaligned(7, k->picked, k->count) || misaligned(3, k->mind, k->label, k->radius, k->aux))
        return fail(FN_EINVAL, "fn_kcenter: misaligned buffer (x, scratch: 16 bytes; picked, count: 8; mind, label, radius, aux: 4)");
    if (k->scratch_bytes < kScratchBytes) return fail(FN_EINVAL, "fn_kcenter: scratch smaller than fn_kcenter_scratch_bytes");
    return 0;
}

int launch_pass(const fn_kcenter* k, const PassArgs& a, int grid, hipStream_t st, const char* where) {
    const dim3 g((unsigned)grid), b(256);
    if (k->d == 128) {
        if (k->metric == 0) hipLaunchKernelGGL((k_kc_pass<128, 0>), g, b, 0, st, a);
        else hipLaunchKernelGGL((k_kc_pass<128, 1>), g, b, 0, st, a);
    } else {
        if (k->metric == 0) hipLaunchKernelGGL((k_kc_pass<256, 0>), g, b, 0, st, a);
        else hipLaunchKernelGGL((k_kc_pass<256, 1>), g, b, 0, st, a);
    }
    return launch_status(where);
}

PassArgs pass_args(const fn_kcenter* k) {
    PassArgs a = {};
    a.x = k->x; a.aux = k->aux; a.mind = k->mind; a.label = k->label; a.picked = k->picked; a.radius = k->radius; a.count = k->count;
    a.n = k->n; a.cap = k->cap; a.first = -1;
    return a;
}

}  // namespace

extern "C" {

int64_t fn_kcenter_scratch_bytes(const fn_kcenter* k) {
    int grid;
    const int rc = check(k, &grid);
    return rc ? rc : kScratchBytes;
}

int fn_kcenter_seed_f32(const fn_kcenter* k, const float* centres, const float* centres_aux, int64_t s, fn_stream_t stream) {
    int grid;
    FN_TRY(check(k, &grid));
    if (s < 0) return fail(FN_EINVAL, "fn_kcenter_seed_f32: negative number of centres");
    if (k->host_count + s > k->cap) return fail(FN_EINVAL, "fn_kcenter_seed_f32: more centres than cap");
    if (s == 0) return 0;
    if (!centres || (k->metric == 1 && !centres_aux) || misaligned(15, centres) || misaligned(3, centres_aux))
        return fail(FN_EINVAL, "fn_kcenter_seed_f32: null or misaligned centres (16 bytes; centres_aux for metric 1: 4)");
    if (!k->picked || !k->radius || !k->count || misaligned(7, k->picked, k->count) || misaligned(3, k->radius))
        return fail(FN_EINVAL, "fn_kcenter_seed_f32: null or misaligned picked, radius or count");
    if (k->n > 0) {
        FN_TRY(check_buffers(k));
        PassArgs a = pass_args(k);
        a.mode = kSeed;
        for (int64_t i = 0; i < s; ++i) {
            a.centre = centres + i * k->d;
            a.centre_aux = centres_aux ? centres_aux + i : nullptr;
            a.seed_index = i;
            FN_TRY(launch_pass(k, a, grid, S(stream), "fn_kcenter_seed_f32 (pass)"));
        }
    }
    hipLaunchKernelGGL(k_kc_seed_close, dim3(1), dim3(256), 0, S(stream), k->picked, k->radius, k->count, s, k->cap);
    return launch_status("fn_kcenter_seed_f32 (close)");
}

int fn_kcenter_pick_f32(const fn_kcenter* k, int64_t first, int64_t n_picks, fn_stream_t stream) {
    int grid;
    FN_TRY(check(k, &grid));
    if (n_picks < 0 || n_picks > k->n - k->host_picks) return fail(FN_EINVAL, "fn_kcenter_pick_f32: k is negative or above the rows not yet picked");
    if (k->host_count + n_picks > k->cap) return fail(FN_EINVAL, "fn_kcenter_pick_f32: more centres than cap");
    if (first < -1 || (k->n > 0 && first >= k->n) || (k->n == 0 && first >= 0)) return fail(FN_EINVAL, "fn_kcenter_pick_f32: first outside [-1, n)");
    if (first >= 0 && k->host_count > 0) return fail(FN_EINVAL, "fn_kcenter_pick_f32: a first row can only be named before any centre (seed or pick)");
    if (k->n == 0 || n_picks == 0) return 0;
    FN_TRY(check_buffers(k));
    Table* const tab = reinterpret_cast<Table*>(k->scratch);
    PassArgs a = pass_args(k);
    a.prev_entries = grid;
    int q = 0;                                                     // launch q writes table q & 1 and reads the other
    if (first < 0) {
        a.mode = kScan;
        a.next = tab;
        FN_TRY(launch_pass(k, a, grid, S(stream), "fn_kcenter_pick_f32 (scan)"));
        q = 1;
    }
    for (int64_t j = 0; j < n_picks; ++j, ++q) {
        a.mode = q == 0 ? kGiven : kTable;
        a.first = q == 0 ? first : -1;
        a.prev = tab + ((q + 1) & 1);
        a.next = tab + (q & 1);
        FN_TRY(launch_pass(k, a, grid, S(stream), "fn_kcenter_pick_f32 (pass)"));
    }
    hipLaunchKernelGGL(k_kc_close, dim3(1), dim3(256), 0, S(stream), tab + ((q + 1) & 1), grid, k->radius, k->count, k->cap);
    return launch_status("fn_kcenter_pick_f32 (close)");
}

}  // extern "C"
