// moments.hip -- first and second moments of a row table x [n, d] (count, column sums, Gram matrix) in fp64, and the affine projection
// of rows onto a few directions, optionally reduced to a squared norm: the two primitives of the chemical-space map (PCA) and of the
// Mahalanobis applicability domain.  A translation unit of its own: nothing shared with the encoder's kernels but fn_internal.h.
//
// fn_rows_moments_f32: two launches, no atomics, no workgroup waits on another.
//   k_moments_blocks  a work item is (super-chunk s, 64 x 64 block (mi <= mj) of the Gram matrix): d = 256 has 10 such blocks, d = 128 has 3.
//                     A super-chunk is FN_MOMENTS_GROUP chunks of FN_MOMENTS_CHUNK rows.  The workgroup (4 waves) stages 128 rows of the
//                     block's two 64-column panels of z = x - shift in LDS (the next 128 rows are in flight in registers meanwhile, 8 or 16
//                     16-byte loads per thread issued back to back and first touched on their way into LDS); wave
//                     w owns the four 16 x 16 tiles of tile row w: per 4 rows one A operand and up to four B operands from LDS, one
//                     fp32-input MFMA (16x16x4) per tile.  A = z[rows][column block of mi], B = z[rows][column block of mj], so the MFMA's
//                     k runs over ROWS: an entry is one fp32 fma chain over the chunk's rows in ascending order.  At every chunk end the
//                     fp32 tiles are added onto fp64 tiles in registers and cleared; at the end of the super-chunk the fp64 tiles go to
//                     the super-chunk's slot in scratch.  Diagonal blocks compute the tiles on and above the diagonal only, and carry the
//                     column sums of their 64 columns (the A operand is the column block: four fp32 add chains per column, rows mod 4).
//   k_moments_fold    one thread per entry on or above the diagonal (and per column sum): the slots in ascending order, then one fp64
//                     addition onto the caller's value when accumulating; the entry below the diagonal is written as a copy.
// The order of every addition depends on n alone.  A workgroup walks items `grid` apart, so the grid decides who computes a slot's block,
// never how.  Items of one super-chunk are dealt to workgroups whose numbers agree modulo 8 (one XCD: its L2 serves the re-reads of the
// super-chunk's rows by the other blocks); speed only.  Rows past n are never read: the load is clamped to the last row, the value dropped.
//
// fn_rows_project_f32: one launch.  A wave keeps two 16-row A operand sets of z in registers (as the nearest-neighbour scan keeps its
// queries) and walks the 16-column tiles of W, each staged once per workgroup in LDS: d/4 MFMAs per row set and tile.  The squared norm
// is a serial fma chain over the tile's 16 columns (lane to lane), carried from tile to tile, so `sq` alone writes no n x k table.
//
// Measured on one MI355X (profiles/chemspace_moments.txt): moments of 1 M rows 1.9 ms (d = 256) / 1.5 ms (d = 128), of
// 65 536 rows 1.4 ms either way -- a call of up to one super-chunk is ONE workgroup's walk per block, so small tables lose to a library
// GEMM; projections 0.24 / 0.12 ms (k = 2) and 2.2 / 0.7 ms (k = d, squared norm only) at 1 M rows.  One setting of the two header
// constants was run.  Measured and dropped: the subtraction next to the load (every load then waited for the one before: 4.1 ms for ANY n
// up to a super-chunk).  Changed with it, not measured apart: the diagonal blocks' `j >= w` inside the common loop.
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

constexpr int kChunk = FN_MOMENTS_CHUNK, kGroup = FN_MOMENTS_GROUP;
constexpr int64_t kSuperRows = (int64_t)kChunk * kGroup;
constexpr int kStep = 128;            // rows staged per step: 32 MFMA k-steps, 8 or 16 16-byte loads per thread in flight under them
constexpr int kLd = 144;              // LDS row stride in floats: two 64-column panels + 16.  144 = 16 mod 64: the four rows of an operand fetch fall on distinct banks
constexpr int kMaxGrid = 2048;
constexpr size_t kMomLds = (size_t)kStep * kLd * sizeof(float);      // 72 KB: two workgroups per CU
constexpr int kWLd = 20;              // LDS row stride of a W tile: 4 rows are 80 = 16 mod 64 floats apart
static_assert(kChunk % 64 == 0 && kChunk <= 1024 && kChunk % kStep == 0, "FN_MOMENTS_CHUNK: a multiple of 64, at most 1024");

struct MomArgs {
    const float *x, *shift;
    double* slots;                    // [supers][d * d + d]
    int64_t n, supers, items;
};

template <int D>
__global__ __launch_bounds__(256) void k_moments_blocks(const MomArgs a) {
    constexpr int MB = D / 64;                                     // 64-column blocks per side
    constexpr int M = MB * (MB + 1) / 2;                           // blocks on and above the diagonal
    constexpr int P = kStep / 16;                                  // 16-byte loads per thread, panel and step: kStep rows x 16 per panel
    extern __shared__ __attribute__((aligned(16))) float zs[];     // [kStep][kLd]
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, h = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);        // the wave: a scalar, so a test on it is a scalar branch
    const int l_row = tid >> 4, l_c4 = (tid & 15) * 4;             // piece (panel q, p) of a step: row l_row + 16 p, floats l_c4 .. + 3 of the panel's row
    for (int64_t item = blockIdx.x; item < a.items; item += gridDim.x) {
        const int64_t within = item % (8 * M);
        const int64_t s = (item / (8 * M)) * 8 + within % 8;
        if (s >= a.supers) continue;                               // (uniform: the last group of eight super-chunks may be short)
        int mi = 0, rem = (int)(within / 8);
        while (rem >= MB - mi) { rem -= MB - mi; ++mi; }
        const int mj = mi + rem;
        const bool diag = mi == mj;
        const int panels = diag ? 1 : 2;
        const int64_t row_begin = s * kSuperRows;
        const int64_t row_end = row_begin + kSuperRows < a.n ? row_begin + kSuperRows : a.n;
        const int64_t steps = (row_end - row_begin + kStep - 1) / kStep;

        float4 sh[2], regs[2][P];
#pragma unroll
        for (int q = 0; q < 2; ++q) sh[q] = (a.shift && q < panels) ? ld4(a.shift + (q ? mj : mi) * 64 + l_c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        // a step's loads are issued back to back and nothing touches them before the step's products are done: the subtraction and the
        // zeros of the rows past row_end happen on the way into LDS (with them next to the load, every load waited for the one before)
        auto fetch = [&](int64_t step) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (q < panels) {
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const int64_t gr = row_begin + step * kStep + l_row + 16 * p;
                        regs[q][p] = ld4(a.x + (gr < a.n ? gr : a.n - 1) * D + (q ? mj : mi) * 64 + l_c4);     // past n: the last row again, dropped in stage()
                    }
                }
        };
        auto stage = [&](int64_t step) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                if (q < panels) {
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const bool in = row_begin + step * kStep + l_row + 16 * p < row_end;
                        const float4 v = regs[q][p];
                        float4 z;
                        z.x = in ? v.x - sh[q].x : 0.f; z.y = in ? v.y - sh[q].y : 0.f; z.z = in ? v.z - sh[q].z : 0.f; z.w = in ? v.w - sh[q].w : 0.f;
                        *reinterpret_cast<float4*>(zs + (l_row + 16 * p) * kLd + q * 64 + l_c4) = z;
                    }
                }
        };

        f32x4 acc[4];
        double acc64[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < 4; ++g) acc64[j][g] = 0.0;
        }
        float cs = 0.f;
        double cs64 = 0.0;

        fetch(0);
        for (int64_t step = 0; step < steps; ++step) {
            __syncthreads();                                       // the step (or item) before has read its rows
            stage(step);
            __syncthreads();
            if (step + 1 < steps) fetch(step + 1);                 // in flight under this step's products
            const int64_t left = row_end - (row_begin + step * kStep);
            const int ksteps = left < kStep ? (int)((left + 3) / 4) : kStep / 4;          // 4-row MFMA steps with a row in them; the rest are zeros and add nothing
            // the two kinds of block as two straight-line bodies: a diagonal block's test `j >= w` inside the common loop put every MFMA in a
            // basic block of its own
            auto products = [&](auto dg, auto whole) {
                constexpr bool DG = decltype(dg)::value, WHOLE = decltype(whole)::value;
                const int kend = WHOLE ? kStep / 4 : ksteps;       // a whole step: a constant the loop is unrolled against
#pragma unroll 8
                for (int kk = 0; kk < kend; ++kk) {
                    const float* rowp = zs + (kk * 4 + h) * kLd;
                    const float av = rowp[w * 16 + r];
                    if (DG) cs += av;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (!DG || j >= w)                         // (wave-uniform)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, rowp[(DG ? 0 : 64) + j * 16 + r], acc[j], 0, 0, 0);
                }
            };
            const bool whole = ksteps == kStep / 4;
            if (diag && whole) products(std::true_type{}, std::true_type{});
            else if (diag) products(std::true_type{}, std::false_type{});
            else if (whole) products(std::false_type{}, std::true_type{});
            else products(std::false_type{}, std::false_type{});
            if ((step + 1) % (kChunk / kStep) == 0 || step + 1 == steps) {            // a chunk ends: fp32 -> fp64, ascending chunks
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc64[j][g] += (double)acc[j][g];
                    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
                cs64 += (double)cs;
                cs = 0.f;
            }
        }
        double* const slot = a.slots + s * ((int64_t)D * D + D);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!diag || j >= w) {
#pragma unroll
                for (int g = 0; g < 4; ++g) slot[(int64_t)(mi * 64 + w * 16 + 4 * h + g) * D + mj * 64 + j * 16 + r] = acc64[j][g];
            }
        if (diag) {                                                // the column's four partial sums (rows mod 4), in order
            const double v0 = __shfl(cs64, r), v1 = __shfl(cs64, r + 16), v2 = __shfl(cs64, r + 32), v3 = __shfl(cs64, r + 48);
            if (h == 0) slot[(int64_t)D * D + mi * 64 + w * 16 + r] = ((v0 + v1) + v2) + v3;
        }
    }
}

// entries [0, d * d): gram (on and above the diagonal; the mirror is a copy), [d * d, d * d + d): sum
__global__ __launch_bounds__(256) void k_moments_fold(const double* __restrict__ slots, int64_t supers, int d, double* sum, double* gram,
                                                      int accumulate) {
    const int64_t total = (int64_t)d * d + d, idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const bool is_sum = idx >= (int64_t)d * d;
    const int j = (int)(idx / d), l = (int)(idx % d);
    if (!is_sum && j > l) return;
    double t = slots[idx];
    for (int64_t s = 1; s < supers; ++s) t += slots[s * total + idx];
    double* const out = is_sum ? sum + (idx - (int64_t)d * d) : gram + idx;
    if (accumulate) t = *out + t;
    *out = t;
    if (!is_sum && j != l) gram[(int64_t)l * d + j] = t;
}

struct ProjArgs {
    const float *x, *shift, *W;
    float *out, *sq;
    int64_t n;
    int k;
};

constexpr int kProjRows = 128;        // per workgroup: two 16-row sets per wave

template <int D>
__global__ __launch_bounds__(256) void k_rows_project(const ProjArgs a) {
    constexpr int T = D / 16;
    __shared__ float wt[D * kWLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, h = lane >> 4, k = a.k;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * 32;
    // A operands: rows row0 + r and row0 + 16 + r (clamped: rows past n are computed and never written), columns 16 t + 4 h + e
    f32x4 za[2][T];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        int64_t ri = row0 + 16 * s + r;
        ri = ri < a.n ? ri : a.n - 1;
        const f32x4* row = reinterpret_cast<const f32x4*>(a.x + ri * D) + h;
#pragma unroll
        for (int t = 0; t < T; ++t) za[s][t] = row[4 * t];
    }
    if (a.shift) {
        const f32x4* srow = reinterpret_cast<const f32x4*>(a.shift) + h;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const f32x4 sv = srow[4 * t];
            za[0][t] -= sv;
            za[1][t] -= sv;
        }
    }
    float sqv[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int tiles = (k + 15) / 16;
    // W[:, 16 ct .. 16 ct + 15] through registers: element e = tid + 256 i is (row e / 16, column e % 16); columns past k: the last column, never written
    float wreg[D / 16];
    auto fetch_w = [&](int ct) {
        const int c = ct * 16 + (tid & 15);
#pragma unroll
        for (int i = 0; i < D / 16; ++i) wreg[i] = a.W[(int64_t)((tid >> 4) + 16 * i) * k + (c < k ? c : k - 1)];
    };
    fetch_w(0);
    for (int ct = 0; ct < tiles; ++ct) {
        __syncthreads();                                           // the tile before has been read
#pragma unroll
        for (int i = 0; i < D / 16; ++i) wt[((tid >> 4) + 16 * i) * kWLd + (tid & 15)] = wreg[i];
        __syncthreads();
        if (ct + 1 < tiles) fetch_w(ct + 1);                       // in flight under this tile's products
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float b = wt[(16 * t + 4 * h + e) * kWLd + r];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(za[0][t][e], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(za[1][t][e], b, acc1, 0, 0, 0);
            }
        const int col = ct * 16 + r;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = s == 0 ? acc0[g] : acc1[g];
                const int64_t row = row0 + 16 * s + 4 * h + g;
                if (a.out && row < a.n && col < k) a.out[row * k + col] = v;
                if (a.sq) {                                        // the 16 lanes of a row all carry the row's chain
                    float q = sqv[s][g];
#pragma unroll
                    for (int cc = 0; cc < 16; ++cc) {
                        const float o = __shfl(v, (lane & 48) + cc);
                        if (ct * 16 + cc < k) q = __builtin_fmaf(o, o, q);
                    }
                    sqv[s][g] = q;
                }
            }
    }
    if (a.sq && r == 0) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = row0 + 16 * s + 4 * h + g;
                if (row < a.n) a.sq[row] = sqv[s][g];
            }
    }
}

// what both moments entry points check; the launch shape is a function of n, d and splits alone, and no result depends on it
int check_moments(const fn_moments* m, int64_t* supers) {
    if (!m || m->n < 0 || m->splits < 0 || m->n >= (1ll << 40)) return fail(FN_EINVAL, "fn_moments: null descriptor, negative size or splits, or n >= 2^40");
    if (m->d != 128 && m->d != 256) return fail(FN_EUNSUPPORTED, "fn_moments: rows are 128 or 256 floats wide");
    *supers = (m->n + kSuperRows - 1) / kSuperRows;
    return 0;
}

int64_t moments_bytes(const fn_moments* m, int64_t supers) { return supers * ((int64_t)m->d * m->d + m->d) * (int64_t)sizeof(double); }

}  // namespace

extern "C" {

int64_t fn_moments_scratch_bytes(const fn_moments* m) {
    int64_t supers;
    const int rc = check_moments(m, &supers);
    return rc ? rc : moments_bytes(m, supers);
}

int fn_rows_moments_f32(const fn_moments* m, fn_stream_t stream) {
    int64_t supers;
    FN_TRY(check_moments(m, &supers));
    if (!m->sum || !m->gram || misaligned(7, m->sum, m->gram)) return fail(FN_EINVAL, "fn_rows_moments_f32: null or misaligned sum or gram (8 bytes)");
    const int64_t entries = (int64_t)m->d * m->d + m->d;
    if (m->n == 0) {
        if (m->accumulate) return 0;
        if (hipMemsetAsync(m->sum, 0, (size_t)m->d * sizeof(double), S(stream)) != hipSuccess ||
            hipMemsetAsync(m->gram, 0, (size_t)m->d * m->d * sizeof(double), S(stream)) != hipSuccess)
            return launch_status("fn_rows_moments_f32 (zero fill)");
        return 0;
    }
    if (!m->x || !m->scratch) return fail(FN_EINVAL, "fn_rows_moments_f32: null buffer (x, scratch)");
    if (misaligned(15, m->x, m->shift, m->scratch)) return fail(FN_EINVAL, "fn_rows_moments_f32: misaligned buffer (x, shift, scratch: 16 bytes)");
    if (m->scratch_bytes < moments_bytes(m, supers)) return fail(FN_EINVAL, "fn_rows_moments_f32: scratch smaller than fn_moments_scratch_bytes");

    const int mb = m->d / 64, blocks = mb * (mb + 1) / 2;
    MomArgs a;
    a.x = m->x; a.shift = m->shift; a.slots = reinterpret_cast<double*>(m->scratch);
    a.n = m->n; a.supers = supers;
    a.items = (supers + 7) / 8 * 8 * blocks;
    int64_t grid = m->splits > 0 ? m->splits : kMaxGrid;
    if (grid > a.items) grid = a.items;
    if (m->d == 128) {
        FN_TRY(allow_lds(k_moments_blocks<128>, kMomLds));
        hipLaunchKernelGGL(k_moments_blocks<128>, dim3((unsigned)grid), dim3(256), kMomLds, S(stream), a);
    } else {
        FN_TRY(allow_lds(k_moments_blocks<256>, kMomLds));
        hipLaunchKernelGGL(k_moments_blocks<256>, dim3((unsigned)grid), dim3(256), kMomLds, S(stream), a);
    }
    FN_TRY(launch_status("fn_rows_moments_f32 (blocks)"));
    hipLaunchKernelGGL(k_moments_fold, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, S(stream), a.slots, supers, m->d, m->sum, m->gram,
                       m->accumulate);
    return launch_status("fn_rows_moments_f32 (fold)");
}

int fn_rows_project_f32(const fn_project* p, fn_stream_t stream) {
    if (!p || p->n < 0 || p->n >= (1ll << 37)) return fail(FN_EINVAL, "fn_rows_project_f32: null descriptor, negative size, or n >= 2^37");
    if (p->d != 128 && p->d != 256) return fail(FN_EUNSUPPORTED, "fn_rows_project_f32: rows are 128 or 256 floats wide");
    if (p->k < 1 || p->k > p->d) return fail(FN_EINVAL, "fn_rows_project_f32: k outside [1, d]");
    if (!p->out && !p->sq) return fail(FN_EINVAL, "fn_rows_project_f32: neither out nor sq is given");
    if (p->n == 0) return 0;
    if (!p->x || !p->W) return fail(FN_EINVAL, "fn_rows_project_f32: null buffer (x, W)");
    if (misaligned(15, p->x, p->shift) || misaligned(3, p->W, p->out, p->sq))
        return fail(FN_EINVAL, "fn_rows_project_f32: misaligned buffer (x, shift: 16 bytes; W, out, sq: 4)");
    ProjArgs a;
    a.x = p->x; a.shift = p->shift; a.W = p->W; a.out = p->out; a.sq = p->sq; a.n = p->n; a.k = p->k;
    const dim3 grid((unsigned)((p->n + kProjRows - 1) / kProjRows));
    if (p->d == 128) hipLaunchKernelGGL(k_rows_project<128>, grid, dim3(256), 0, S(stream), a);
    else hipLaunchKernelGGL(k_rows_project<256>, grid, dim3(256), 0, S(stream), a);
    return launch_status("fn_rows_project_f32");
}

}  // extern "C"
