// row_sample.hip -- fn_select_rows_u8 / fn_sample_rows_u8: an exact-count sample of rows without replacement, drawn on the device.
// Of the n real rows of a table of `cap` rows, k = (int)((double)n * keep_frac) are kept: row i < n gets byte 1 iff fewer than k rows
// j < n have (key_j, j) < (key_i, i) lexicographically -- the k smallest keys, ties broken by row index -- and the padding rows
// n <= i < cap get 1.  The keys are the caller's (select) or word i % 4 of Philox block offset + i / 4 (sample: the convention of
// fn_dropout_act_f32).  n may live in device memory (a padded batch of a captured step knows its real rows only there).
//
// One workgroup of 1024 threads: a radix select of the k-th smallest key in four 8-bit passes (per-wave histograms in LDS, one scan
// of the 256 bins per pass), then ONE pass over all cap rows in index order that counts the rows tying with the pivot (block-wide
// prefix count with a running carry) and writes the bytes.  Up to cap = 16384 (the pretrain shape: 14 k atoms) a thread HOLDS its
// keys -- four quads, sixteen VGPRs -- across the five passes: on one CU the Philox blocks are the kernel's arithmetic (two quarter-rate
// 32 x 32 -> 64 multiplies per round), and regenerating them per pass cost five times what drawing them once costs.  Registers, not
// LDS: the keys are only ever read by the thread that drew them (56 KB of LDS would buy nothing).  Beyond that capacity the same code
// re-reads / regenerates per pass and serves any cap up to 2^24 by looping.  -Rpass-analysis=kernel-resource-usage, holding / looping
// instances: 56 / 66 VGPRs, 16456 B of LDS (the sixteen per-wave histograms), no scratch, 8 / 7 waves per SIMD.  In the captured
// pretrain step (B = 512, capacity 13872 atoms) holding the keys took the masked step's surcharge from 21.3 to 13.4 us.
#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

constexpr int kSelThreads = 1024, kSelWaves = kSelThreads / 64;
constexpr int kHeld = 4;                                           // quads a thread holds in registers (HELD instances)
constexpr int64_t kHeldCap = (int64_t)4 * kHeld * kSelThreads;     // rows those cover

struct SelArgs {
    const uint32_t* keys;            // select: [cap]; sample: null
    uint64_t seed, offset;
    const uint64_t* offset_dev;      // nullable: added to offset
    int64_t cap, n;
    const int32_t* n_dev;            // nullable: the real row count, clamped to [0, cap]
    double keep_frac;
    uint8_t* out;                    // [cap]
};

template <bool GEN>
__device__ __forceinline__ uint4 load_quad(const SelArgs& A, int64_t q, uint64_t off, int64_t n) {
    if (GEN) return philox4x32(off + (uint64_t)q, A.seed);
    const int64_t i = q * 4;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) r.x = A.keys[i];
    if (i + 1 < n) r.y = A.keys[i + 1];
    if (i + 2 < n) r.z = A.keys[i + 2];
    if (i + 3 < n) r.w = A.keys[i + 3];
    return r;
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(v, d);
        if (lane >= d) v += u;
    }
    return v;
}

// HELD (the launcher's word that cap <= kHeldCap): thread t keeps the keys of quads t, t + 1024, .. in registers
template <bool GEN, bool HELD>
__global__ __launch_bounds__(kSelThreads) void k_select_rows(SelArgs A) {
    __shared__ uint32_t hist[kSelWaves][256];
    __shared__ uint32_t wsum[kSelWaves];
    __shared__ uint32_t pick[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t n = A.n_dev ? (int64_t)*A.n_dev : A.n;
    n = n < 0 ? 0 : (n > A.cap ? A.cap : n);
    int64_t k = (int64_t)((double)n * A.keep_frac);       // Python's int(n * keep_frac): the same IEEE double product, truncated
    k = k < 0 ? 0 : (k > n ? n : k);
    const uint64_t off = A.offset + (A.offset_dev ? *A.offset_dev : 0ull);
    const int64_t nq = (n + 3) / 4;
    const bool all = k >= n, none = k == 0 && n > 0;
    uint4 held[kHeld];
    if (HELD && !all && !none) {
#pragma unroll
        for (int u = 0; u < kHeld; ++u) {
            const int64_t q = tid + (int64_t)u * kSelThreads;
            held[u] = q < nq ? load_quad<GEN>(A, q, off, n) : make_uint4(0u, 0u, 0u, 0u);
        }
    }

    uint32_t pivot = 0u, ties = 0u;       // keep key < pivot, and the first `ties` rows (by index) with key == pivot
    if (!all && !none) {
        uint32_t prefix = 0u, r = (uint32_t)(k - 1);       // the rank still looked for among the keys that share `prefix`
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int b = tid; b < kSelWaves * 256; b += kSelThreads) (&hist[0][0])[b] = 0u;
            __syncthreads();
            auto tally = [&](int64_t q, const uint4& kq) {
                const uint32_t key[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (q * 4 + j < n && (shift == 24 || (key[j] >> (shift + 8)) == prefix)) atomicAdd(&hist[wave][(key[j] >> shift) & 255u], 1u);
            };
            if (HELD) {
#pragma unroll
                for (int u = 0; u < kHeld; ++u) {
                    const int64_t q = tid + (int64_t)u * kSelThreads;
                    if (q < nq) tally(q, held[u]);
                }
            } else {
                for (int64_t q = tid; q < nq; q += kSelThreads) tally(q, load_quad<GEN>(A, q, off, n));
            }
            __syncthreads();
            uint32_t c = 0u, incl = 0u;
            if (tid < 256) {
#pragma unroll
                for (int w = 0; w < kSelWaves; ++w) c += hist[w][tid];
                incl = wave_incl_scan(c, lane);
                if (lane == 63) wsum[wave] = incl;
            }
            __syncthreads();
            if (tid < 256) {
                uint32_t base = 0u;
                for (int w = 0; w < wave; ++w) base += wsum[w];
                const uint32_t excl = base + incl - c;
                if (c && excl <= r && r < excl + c) { pick[0] = (uint32_t)tid;  pick[1] = r - excl; }
            }
            __syncthreads();
            prefix = (prefix << 8) | pick[0];
            r = pick[1];
        }
        pivot = prefix;
        ties = r + 1u;
    }

    // index order: thread t of round `base` owns rows 4 (base + t) .. + 3; `run` = ties in the rounds before this one
    const int64_t ncq = (A.cap + 3) / 4;
    const bool aligned = ((uintptr_t)A.out & 3) == 0;
    uint32_t run = 0u;
    auto emit = [&](int64_t base, const uint4& mine) {        // mine: the held keys of this round's quad (HELD instances)
        const int64_t q = base + tid, i0 = q * 4;
        const bool scan = !all && !none && base < nq;          // block-uniform
        uint32_t key[4] = {0u, 0u, 0u, 0u};
        uint32_t cnt = 0u, excl = 0u;
        if (scan) {
            if (q < nq) {
                const uint4 kq = HELD ? mine : load_quad<GEN>(A, q, off, n);
                key[0] = kq.x;  key[1] = kq.y;  key[2] = kq.z;  key[3] = kq.w;
#pragma unroll
                for (int j = 0; j < 4; ++j) cnt += (i0 + j < n && key[j] == pivot) ? 1u : 0u;
            }
            const uint32_t incl = wave_incl_scan(cnt, lane);
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t wbase = 0u, total = 0u;
#pragma unroll
            for (int w = 0; w < kSelWaves; ++w) { const uint32_t s = wsum[w];  wbase += w < wave ? s : 0u;  total += s; }
            excl = run + wbase + incl - cnt;
            run += total;
            __syncthreads();
        }
        if (q < ncq) {
            uint32_t word = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t b;
                if (i0 + j >= n || all) b = 1u;
                else if (none) b = 0u;
                else if (key[j] < pivot) b = 1u;
                else if (key[j] == pivot) b = excl++ < ties ? 1u : 0u;
                else b = 0u;
                word |= b << (8 * j);
            }
            if (aligned && i0 + 4 <= A.cap) *reinterpret_cast<uint32_t*>(A.out + i0) = word;
            else
                for (int j = 0; j < 4 && i0 + j < A.cap; ++j) A.out[i0 + j] = (uint8_t)((word >> (8 * j)) & 0xffu);
        }
    };
    if (HELD) {                                               // cap <= kHeldCap: at most kHeld rounds
#pragma unroll
        for (int u = 0; u < kHeld; ++u)
            if ((int64_t)u * kSelThreads < ncq) emit((int64_t)u * kSelThreads, held[u]);
    } else {
        for (int64_t base = 0; base < ncq; base += kSelThreads) emit(base, make_uint4(0u, 0u, 0u, 0u));
    }
}

int select_rows(const char* who, const uint32_t* keys, bool gen, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t cap,
                int64_t n, const int32_t* n_dev, double keep_frac, uint8_t* out, fn_stream_t stream) {
    if (cap < 0 || cap > (1 << 24)) return fail(FN_EINVAL, who);
    if (!(keep_frac >= 0.0 && keep_frac <= 1.0)) return fail(FN_EINVAL, who);
    if (!n_dev && (n < 0 || n > cap)) return fail(FN_EINVAL, who);
    if (cap == 0) return 0;
    if (!out || (!gen && !keys)) return fail(FN_EINVAL, who);
    SelArgs A{keys, seed, offset, offset_dev, cap, n, n_dev, keep_frac, out};
    const bool held = cap <= kHeldCap;
    if (gen && held) hipLaunchKernelGGL((k_select_rows<true, true>), dim3(1), dim3(kSelThreads), 0, S(stream), A);
    else if (gen) hipLaunchKernelGGL((k_select_rows<true, false>), dim3(1), dim3(kSelThreads), 0, S(stream), A);
    else if (held) hipLaunchKernelGGL((k_select_rows<false, true>), dim3(1), dim3(kSelThreads), 0, S(stream), A);
    else hipLaunchKernelGGL((k_select_rows<false, false>), dim3(1), dim3(kSelThreads), 0, S(stream), A);
    return launch_status(who);
}
}  // namespace

extern "C" {
int fn_select_rows_u8(const uint32_t* keys, int64_t cap, int64_t n, const int32_t* n_dev, double keep_frac, uint8_t* out, fn_stream_t stream) {
    return select_rows("fn_select_rows_u8: cap in [0, 2^24], n in [0, cap], keep_frac in [0, 1], non-null keys / out", keys, false, 0, 0, nullptr,
                       cap, n, n_dev, keep_frac, out, stream);
}
int fn_sample_rows_u8(uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t cap, int64_t n, const int32_t* n_dev, double keep_frac,
                      uint8_t* out, fn_stream_t stream) {
    return select_rows("fn_sample_rows_u8: cap in [0, 2^24], n in [0, cap], keep_frac in [0, 1], non-null out", nullptr, true, seed, offset,
                       offset_dev, cap, n, n_dev, keep_frac, out, stream);
}
}  // extern "C"
