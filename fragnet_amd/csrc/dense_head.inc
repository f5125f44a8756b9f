// Dense layers of the prediction heads on the fp32 matrix cores, with the element-wise work around them fused in
// (included into the anonymous namespace of head.hip behind head_act.inc; the address-space helpers it uses: fn_internal.h).
//
// Reference: FTHead1-5 (model/gat/gat2.py:569-751) are stacks of  act(dropout(Linear(x)))  on [molecules, width] with
// molecules ~ 512 and widths 128 ... 1024: ~1 GFLOP per product, operands that fit the L2.  At that size the fp32 MFMA
// rate (64 FLOP/clk/SIMD) and the fixed cost of a kernel (cold L2 after the kernel boundary, ~7 us) set the pace, not
// operand reuse, so the kernels here have no workgroup-shared tile and no barrier in the main loop; they aim at many
// independent waves and at two workgroups per CU.  One family computes   OUT[i][j] = sum_r A(i, r) B(r, j)   for the
// three products of a layer
//     forward          Y  = X W^T        i = row,         j = out feature, r = in feature    (both operands run along r)
//     input gradient   gX = gy W         i = row,         j = in feature,  r = out feature   (A along r, B along j)
//     weight gradient  dW = gy^T X       i = out feature, j = in feature,  r = row           (both operands run ACROSS r)
// and every operand piece is one 16-byte global load per lane:
//   * an operand that runs along r must reach lane (n, g) as the four r = r0 + 4g + 0..3 of row n (MFMA q of the step
//     takes .q).  Loaded that way an instruction touches 64 different cache lines, so the wave loads 64-byte row pieces
//     with 4 neighbouring lanes per row instead and turns them into the operand layout through a wave-private,
//     XOR-swizzled LDS slab (no barrier: one wave's LDS instructions execute in order);
//   * an operand that runs across r gives lane (n, g) the four COLUMNS 4n .. 4n+3 of row r0 + g (or of rows r0 + 4g + q
//     against an along-r partner): component q feeds the accumulator of the output columns (rows) {4n + q}, i.e. the
//     16 x 16 MFMA tiles interleave with stride 4 instead of being contiguous -- no transposition anywhere, every load a
//     full 256-byte run per 16 lanes, and the weight gradient needs no transposed copy of gy.
// A workgroup = 8 waves that split the reduction of ONE output tile (32 x 64; 64 x 64 for the weight gradient) eight ways
// (wave w takes the r-steps w, w+8, ...: neighbouring waves read neighbouring pieces of the same cache lines), keeps the
// next step's pieces in flight in registers, and adds the eight partial tiles through LDS in a fixed order (deterministic).
// A product with fewer than 192 such tiles uses half-width tiles (32 x 32 / 64 x 32: NC = 2, dense_dw_narrow) so that the chip is occupied.
// Fused:  bias + relu(dropout(.)) (the Philox stream of fn_dropout_act_f32) in the forward epilogue;  the backward of the
// layer BELOW's relu(dropout(.)) in the input-gradient epilogue (gX is gated by the layer input X, which is that layer's
// saved output: positive exactly where the element was kept and passed the ReLU), so both gradient products read an
// already gated gy;  the bias gradient (column sums of gy) in the weight-gradient tiles of the first tile column.
constexpr int kDnThreads = 512, kDnWaves = 8, kDnCols = 64, kDnPart = 32 * 64;
constexpr int kDnLdsBytes = kDnWaves * kDnPart * 4;       // 64 KB: eight 32x64 partial tiles = four 64x64 ones; the slabs alias it
constexpr int kDnSlabFwd = 96 * 16, kDnSlabDx = 32 * 16;  // floats per wave: (32 + 64) rows x 16 r  /  32 rows x 16 r
enum { DN_FWD = 0, DN_DX = 1, DN_DW = 2 };

struct DenseArgs {
    // forward: A = X [M,K], Bsrc = W [N,K];   dX: A = gy [M,N], Bsrc = W [N,K], Z = X [M,K];   dW: A = gy [M,N], Bsrc = X [M,K]
    const float* A;
    const float* Z;          // dX: gates the OUTPUT, gX = Z > 0 ? gX * gate_scale : 0 (null: no gate)
    const float* Bsrc;
    const float* bias;       // forward only, nullable
    float* OUT;              // Y [M,N] / gX [M,K] / dW [N,K]
    float* db;               // dW: [N] bias gradient (nullable)
    int I, J, R;             // output rows, output columns, reduction length
    int I_out;               // dX: rows [I, I_out) of OUT are written as 0 (padding rows of a static-shape batch); else 0
    int lda, ldb;            // row strides (floats) of A's and Bsrc's arrays
    float gate_scale;
    fn_act_epilogue act;     // forward: y != null => OUT = relu?(dropout(.)) with act.p / seed / offset (applied in place)
    fn_head_act hact;        // instances with a head activation kind (HA >= 0, head_act.inc): forward: this layer's; dX: the layer below's
    int tiles_i, tiles_j, first_block;
};
struct DensePair { DenseArgs a, b; int a_narrow, b_narrow; };      // one launch, two products (the two gradient products of a layer); a_narrow: 64 x 32 weight-gradient tiles

template <int MODE> struct DnFrag;
template <> struct DnFrag<DN_FWD> { float4 a[2], b[4]; };           // 16 r of 32 + 64 rows, 4 lanes per row
template <> struct DnFrag<DN_DX> { float4 a[2], b[4]; };            // 16 r: 32 rows of gy, 4 lanes per row; 4 rows of W per lane group
template <> struct DnFrag<DN_DW> { float4 a[2], b[2]; };            // 8 r: 2 rows of gy and X per lane group

typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ld2(const glb_f* p) {
    const f32x2 v = *reinterpret_cast<const FN_GLB f32x2*>(p);
    return make_float2(v.x, v.y);
}
__device__ __forceinline__ void st2s(lds_f* p, float a, float b) { *reinterpret_cast<FN_LDS f32x2*>(p) = (f32x2){a, b}; }

// NC = 16-column groups of a forward / input-gradient tile: 4 (32 x 64) or 2 (32 x 32, for products with too few tiles to
// occupy the chip; the input-gradient's W pieces are then 8-byte loads of columns 2n, 2n+1)
// HA: -1 the ReLU path above (act / Z + gate_scale); >= 0 an activation kind of head_act.inc (T.hact) in the forward / input-gradient epilogue
template <int MODE, int NC = 4, int HA = -1>
__device__ __forceinline__ void dense_tile(const DenseArgs& T, int blk, lds_f* smem) {
    using Fr = DnFrag<MODE>;
    static_assert(NC == 4 || (NC == 2 && MODE != DN_DW), "narrow tiles exist for the forward and input-gradient products");
    constexpr int TC = 16 * NC;                           // tile columns
    constexpr int TR = MODE == DN_DW ? 64 : 32;           // tile rows
    constexpr int SL = MODE == DN_DW ? 8 : 16;            // r per step
    constexpr int NACC = MODE == DN_DW ? 16 : 2 * NC;
    constexpr int D = 2;                                  // steps in flight per wave.  (Round 4: six / eight in flight -- the whole share of a wave of the
                                                          // 1024-long reductions -- in launches of one workgroup per CU, 196-218 registers, measured
                                                          // SLOWER: 1024 x 1024 forward 16.5 -> 21.0 us, 1024 x 512 10.0 -> 12.0, the 128-workgroup
                                                          // gradient launch 9.8 -> 11.7: the launches are not round-trip-count bound)
    const int tid = threadIdx.x, l = tid & 63, n = l & 15, g = l >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ti = blk / T.tiles_j, tj = blk - ti * T.tiles_j;
    const int i0 = ti * TR, j0 = tj * TC;
    const int I = T.I, J = T.J, R = T.R, lda = T.lda, ldb = T.ldb;
    const int nsteps = (R + SL - 1) / SL;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const glb_f* Ab = G(T.A);
    const glb_f* Bb = G(T.Bsrc);
    lds_f* slab = smem + wv * (MODE == DN_FWD ? kDnSlabFwd : kDnSlabDx);      // this wave's staging rows (sized for NC = 4)
    // Element offsets are 32 bits (arrays stay below 2^30 floats, checked on the host).  Rows past the end of an along-r
    // operand are clamped: they only feed outputs that are never stored.  r past R loads zeros.
    constexpr unsigned kBad = 0xffffffffu;
    constexpr int CW = MODE == DN_DX ? NC : 4;            // columns per lane of an across-r operand piece
    const unsigned bo = MODE != DN_FWD && j0 + CW * n < J ? (unsigned)(MODE == DN_DX ? 4 * g : g) * ldb + j0 + CW * n : kBad;   // J % 4 == 0
    const unsigned ao = MODE == DN_DW && i0 + 4 * n < I ? (unsigned)g * lda + i0 + 4 * n : kBad;                               // I % 4 == 0
    auto load = [&](Fr& f, int s) {
        if constexpr (MODE != DN_DW) {
            const unsigned r = 16u * s + 4 * (l & 3);
            const bool rok = (int)r < R;                   // R % 4 == 0
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                f.a[k] = zero4;
                if (rok) f.a[k] = ld4(Ab + ((unsigned)max(min(i0 + 16 * k + (l >> 2), I - 1), 0) * lda + r));
            }
            if constexpr (MODE == DN_FWD) {
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    f.b[k] = zero4;
                    if (rok) f.b[k] = ld4(Bb + ((unsigned)min(j0 + 16 * k + (l >> 2), J - 1) * ldb + r));
                }
            } else {
                const bool bok = 16 * s + 4 * g < R && bo != kBad;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f.b[q] = zero4;
                    if (bok) {
                        if constexpr (NC == 4) f.b[q] = ld4(Bb + (bo + (16u * s + q) * ldb));
                        else { const float2 h2 = ld2(Bb + (bo + (16u * s + q) * ldb));  f.b[q].x = h2.x;  f.b[q].y = h2.y; }
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const unsigned rr = 8u * s + 4 * k;
                const bool rok = (int)rr + g < R;
                f.a[k] = zero4;  f.b[k] = zero4;
                if (rok && ao != kBad) f.a[k] = ld4(Ab + (ao + rr * lda));
                if (rok && bo != kBad) f.b[k] = ld4(Bb + (bo + rr * ldb));
            }
        }
    };
    // along-r pieces -> the wave's slab.  Row x (4 pieces of 16 bytes) keeps piece p at slot p ^ ((x >> 2) & 3): the 16 lanes
    // of a ds_read_b128 / ds_write_b128 phase then cover 16 different 16-byte bank groups, both ways.
    auto stage = [&](Fr& f) {
        __builtin_amdgcn_wave_barrier();
        if constexpr (MODE != DN_DW) {
            const int slot = ((l & 3) ^ (l >> 4)) * 4;
#pragma unroll
            for (int k = 0; k < 2; ++k) st4s(slab + (16 * k + (l >> 2)) * 16 + slot, f.a[k]);
            if constexpr (MODE == DN_FWD) {
#pragma unroll
                for (int k = 0; k < NC; ++k) st4s(slab + (32 + 16 * k + (l >> 2)) * 16 + slot, f.b[k]);
            }
        }
        __builtin_amdgcn_wave_barrier();
    };

    f32x4 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 dbacc = zero4;                                   // dW: sum over this lane's rows r of gy[r][i0 + 4n .. + 3]
    auto mfma = [&](Fr& f) {
        if constexpr (MODE == DN_FWD) {                     // acc[t][u]: rows 16t + ., columns 16u + .
            const int slot = (g ^ ((n >> 2) & 3)) * 4;
            float4 a[2], b[NC];
#pragma unroll
            for (int t = 0; t < 2; ++t) a[t] = ld4s(slab + (16 * t + n) * 16 + slot);
#pragma unroll
            for (int u = 0; u < NC; ++u) b[u] = ld4s(slab + (32 + 16 * u + n) * 16 + slot);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < NC; ++u) {
                    DN_MFMA(acc[NC * t + u], a[t].x, b[u].x);  DN_MFMA(acc[NC * t + u], a[t].y, b[u].y);
                    DN_MFMA(acc[NC * t + u], a[t].z, b[u].z);  DN_MFMA(acc[NC * t + u], a[t].w, b[u].w);
                }
        } else if constexpr (MODE == DN_DX) {               // acc[t][q']: rows 16t + ., columns 4. + q';  MFMA q pairs a.q with row q of B
            const int slot = (g ^ ((n >> 2) & 3)) * 4;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float4 a = ld4s(slab + (16 * t + n) * 16 + slot);
                const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    DN_MFMA(acc[NC * t + 0], av[q], f.b[q].x);  DN_MFMA(acc[NC * t + 1], av[q], f.b[q].y);
                    if constexpr (NC == 4) { DN_MFMA(acc[4 * t + 2], av[q], f.b[q].z);  DN_MFMA(acc[4 * t + 3], av[q], f.b[q].w); }
                }
            }
        } else {                                            // acc[q][q']: rows 4. + q, columns 4. + q'
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float av[4] = {f.a[k].x, f.a[k].y, f.a[k].z, f.a[k].w};
                dbacc.x += av[0];  dbacc.y += av[1];  dbacc.z += av[2];  dbacc.w += av[3];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    DN_MFMA(acc[4 * q + 0], av[q], f.b[k].x);  DN_MFMA(acc[4 * q + 1], av[q], f.b[k].y);
                    DN_MFMA(acc[4 * q + 2], av[q], f.b[k].z);  DN_MFMA(acc[4 * q + 3], av[q], f.b[k].w);
                }
            }
        }
    };

    Fr f[D];
#pragma unroll
    for (int d = 0; d < D; ++d) load(f[d], wv + kDnWaves * d);
    for (int s = wv; s < nsteps; s += kDnWaves * D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool on = s + kDnWaves * d < nsteps;      // wave-uniform
            if (on && MODE != DN_DW) stage(f[d]);
            if (MODE == DN_FWD) load(f[d], s + kDnWaves * (d + D));         // its registers are free once the slab holds them
            if (on) mfma(f[d]);
            if (MODE != DN_FWD) load(f[d], s + kDnWaves * (d + D));
        }
    }
    if (MODE != DN_DW) __syncthreads();                     // the partial tiles below overwrite other waves' slabs

    // ---- bias gradient: over the lane groups g (fixed order), then over the eight waves
    if (MODE == DN_DW && T.db && tj == 0) {
        float4 v = dbacc;
        v.x += __shfl_xor(v.x, 16);  v.y += __shfl_xor(v.y, 16);  v.z += __shfl_xor(v.z, 16);  v.w += __shfl_xor(v.w, 16);
        v.x += __shfl_xor(v.x, 32);  v.y += __shfl_xor(v.y, 32);  v.z += __shfl_xor(v.z, 32);  v.w += __shfl_xor(v.w, 32);
        if (l < 16) st4s(smem + wv * 64 + 4 * n, v);
        __syncthreads();
        if (tid < 64 && i0 + tid < I) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < kDnWaves; ++w) s += smem[w * 64 + tid];
            G(T.db)[i0 + tid] = s;
        }
        __syncthreads();
    }
    // ---- partial tiles -> LDS (plain row-major [rows][64]) -> summed in wave order, epilogue, coalesced 16-byte stores
    if (MODE != DN_DW) {
        lds_f* part = smem + wv * (32 * TC);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 16 * t + 4 * g + e;
                if constexpr (MODE == DN_FWD) {
#pragma unroll
                    for (int u = 0; u < NC; ++u) part[row * TC + 16 * u + n] = acc[NC * t + u][e];
                } else if constexpr (NC == 4) {
                    st4s(part + row * TC + 4 * n, make_float4(acc[4 * t][e], acc[4 * t + 1][e], acc[4 * t + 2][e], acc[4 * t + 3][e]));
                } else {
                    st2s(part + row * TC + 2 * n, acc[2 * t][e], acc[2 * t + 1][e]);
                }
            }
        __syncthreads();
    } else {                                                // 64x64 tiles: waves 4..7 hand theirs to waves 0..3 first
        lds_f* part = smem + (wv & 3) * (2 * kDnPart);
        if (wv >= 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    st4s(part + (4 * (4 * g + e) + q) * kDnCols + 4 * n,
                         make_float4(acc[4 * q][e], acc[4 * q + 1][e], acc[4 * q + 2][e], acc[4 * q + 3][e]));
        }
        __syncthreads();
        if (wv < 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    lds_f* p = part + (4 * (4 * g + e) + q) * kDnCols + 4 * n;
                    const float4 o = ld4s(p);
                    st4s(p, make_float4(acc[4 * q][e] + o.x, acc[4 * q + 1][e] + o.y, acc[4 * q + 2][e] + o.z, acc[4 * q + 3][e] + o.w));
                }
        }
        __syncthreads();
    }
    const bool act_on = HA < 0 && MODE == DN_FWD && T.act.y != nullptr;
    const float p = T.act.p, ik = p < 1.f ? 1.f / (1.f - p) : 0.f;
    const uint64_t rng = act_on && p > 0.f ? T.act.offset + (T.act.offset_dev ? *T.act.offset_dev : 0) : 0;
    HactRun hr{};
    if constexpr (HA >= 0 && MODE != DN_DW) hr = hact_run(T.hact, HA);
    float dslope = 0.f;
    glb_f* OUT = G(T.OUT);
    constexpr int NP = MODE == DN_DW ? 4 : kDnWaves, PSZ = MODE == DN_DW ? 2 * kDnPart : 32 * TC, Q4 = TC / 4;
#pragma unroll
    for (int rep = 0; rep < TR / 32; ++rep) {
        const int e = tid + rep * kDnThreads, row = e / Q4, c4 = e % Q4;
        if (NC == 2 && e >= 32 * Q4) break;                 // narrow tile: 256 pieces
        const int gi = i0 + row, gj = j0 + 4 * c4;
        float4 v = ld4s(smem + row * TC + 4 * c4);
#pragma unroll
        for (int w = 1; w < NP; ++w) {
            const float4 o = ld4s(smem + w * PSZ + row * TC + 4 * c4);
            v.x += o.x;  v.y += o.y;  v.z += o.z;  v.w += o.w;
        }
        if (MODE == DN_DX && gi >= I && gi < T.I_out && gj < J) st4(OUT + (size_t)gi * J + gj, make_float4(0.f, 0.f, 0.f, 0.f));
        if (gi < I && gj < J) {                             // J % 4 == 0
            if (HA < 0 && MODE == DN_DX && T.Z) {           // backward of the layer below's relu(dropout(.))
                const float4 z = ld4(G(T.Z) + (size_t)gi * J + gj);
                const float gs = T.gate_scale;
                v = make_float4(z.x > 0.f ? v.x * gs : 0.f, z.y > 0.f ? v.y * gs : 0.f, z.z > 0.f ? v.z * gs : 0.f, z.w > 0.f ? v.w * gs : 0.f);
            }
            if constexpr (HA >= 0 && MODE == DN_DX)         // backward of the layer below's activation kind (its saved argument u)
                v = hact_bwd4<HA>(T.hact, hr, v, ld4(G(T.hact.pre) + (size_t)gi * J + gj), (uint64_t)gi * J + gj, dslope);
            if (MODE == DN_FWD && T.bias) {
                const float4 bb = ld4(G(T.bias) + gj);
                v.x += bb.x;  v.y += bb.y;  v.z += bb.z;  v.w += bb.w;
            }
            if constexpr (HA >= 0 && MODE == DN_FWD) {
                float4 u;
                v = hact_fwd4<HA>(T.hact, hr, v, (uint64_t)gi * J + gj, u);
                st4(G(T.hact.pre) + (size_t)gi * J + gj, u);
            }
            if (act_on) {
                if (p > 0.f) {
                    const uint4 rnd = philox4x32(rng + ((uint64_t)gi * J + gj) / 4, T.act.seed);
                    v.x *= keep_scale(rnd.x, p, ik);  v.y *= keep_scale(rnd.y, p, ik);
                    v.z *= keep_scale(rnd.z, p, ik);  v.w *= keep_scale(rnd.w, p, ik);
                }
                if (T.act.relu) { v.x = fmaxf(v.x, 0.f);  v.y = fmaxf(v.y, 0.f);  v.z = fmaxf(v.z, 0.f);  v.w = fmaxf(v.w, 0.f); }
            }
            st4(OUT + (size_t)gi * J + gj, v);
        }
    }
    if constexpr (HA == FN_ACT_PRELU && MODE == DN_DX) hact_block_partial<kDnWaves>(dslope, T.hact.part, blk, smem);
}

// Weight-gradient tiles of 64 x 32 for layers whose 64 x 64 tiling gives too few workgroups (N = 1024, K = 128: 32 tiles; N = 128,
// K = 256: 8 -- the launch then waits for those few workgroups' MFMA chains): the X pieces are 8-byte loads of columns
// 2n, 2n+1, component q' feeds the accumulators of the output columns {2n + q'}; eight 8-KB partial tiles fit the 64 KB at once.
struct DnFragNarrow { float4 a[2]; float2 b[2]; };

__device__ __forceinline__ void dense_dw_narrow(const DenseArgs& T, int blk, lds_f* smem) {
    const int tid = threadIdx.x, l = tid & 63, n = l & 15, g = l >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ti = blk / T.tiles_j, tj = blk - ti * T.tiles_j;
    const int i0 = ti * 64, j0 = tj * 32;
    const int I = T.I, J = T.J, R = T.R, lda = T.lda, ldb = T.ldb;
    const int nsteps = (R + 7) / 8;
    const glb_f* Ab = G(T.A);
    const glb_f* Bb = G(T.Bsrc);
    constexpr unsigned kBad = 0xffffffffu;
    const unsigned ao = i0 + 4 * n < I ? (unsigned)g * lda + i0 + 4 * n : kBad;      // I % 4 == 0
    const unsigned bo = j0 + 2 * n < J ? (unsigned)g * ldb + j0 + 2 * n : kBad;      // J % 4 == 0
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load = [&](DnFragNarrow& f, int s) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned rr = 8u * s + 4 * k;
            const bool rok = (int)rr + g < R;
            f.a[k] = zero4;  f.b[k] = make_float2(0.f, 0.f);
            if (rok && ao != kBad) f.a[k] = ld4(Ab + (ao + rr * lda));
            if (rok && bo != kBad) f.b[k] = ld2(Bb + (bo + rr * ldb));
        }
    };
    f32x4 acc[8];                                           // acc[2q + q']: rows 4. + q, columns 2. + q'
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 dbacc = zero4;
    DnFragNarrow f[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) load(f[d], wv + kDnWaves * d);
    for (int s = wv; s < nsteps; s += kDnWaves * 2) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
            if (s + kDnWaves * d < nsteps) {                // wave-uniform
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float av[4] = {f[d].a[k].x, f[d].a[k].y, f[d].a[k].z, f[d].a[k].w};
                    dbacc.x += av[0];  dbacc.y += av[1];  dbacc.z += av[2];  dbacc.w += av[3];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        DN_MFMA(acc[2 * q + 0], av[q], f[d].b[k].x);  DN_MFMA(acc[2 * q + 1], av[q], f[d].b[k].y);
                    }
                }
            }
            load(f[d], s + kDnWaves * (d + 2));
        }
    }
    if (T.db && tj == 0) {                                  // bias gradient, as in dense_tile
        float4 v = dbacc;
        v.x += __shfl_xor(v.x, 16);  v.y += __shfl_xor(v.y, 16);  v.z += __shfl_xor(v.z, 16);  v.w += __shfl_xor(v.w, 16);
        v.x += __shfl_xor(v.x, 32);  v.y += __shfl_xor(v.y, 32);  v.z += __shfl_xor(v.z, 32);  v.w += __shfl_xor(v.w, 32);
        if (l < 16) st4s(smem + wv * 64 + 4 * n, v);
        __syncthreads();
        if (tid < 64 && i0 + tid < I) {
            float sum = 0.f;
#pragma unroll
            for (int w = 0; w < kDnWaves; ++w) sum += smem[w * 64 + tid];
            G(T.db)[i0 + tid] = sum;
        }
        __syncthreads();
    }
    lds_f* part = smem + wv * kDnPart;                     // [64][32] per wave
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) st2s(part + (4 * (4 * g + e) + q) * 32 + 2 * n, acc[2 * q][e], acc[2 * q + 1][e]);
    __syncthreads();
    const int row = tid >> 3, c4 = tid & 7;
    float4 v = ld4s(smem + row * 32 + 4 * c4);
#pragma unroll
    for (int w = 1; w < kDnWaves; ++w) {
        const float4 o = ld4s(smem + w * kDnPart + row * 32 + 4 * c4);
        v.x += o.x;  v.y += o.y;  v.z += o.z;  v.w += o.w;
    }
    const int gi = i0 + row, gj = j0 + 4 * c4;
    if (gi < I && gj < J) st4(G(T.OUT) + (size_t)gi * J + gj, v);
}

// ---- the forward product of a TALL input (>= 192 tiles of 64 x 128: 1536+ rows at N = 1024) on workgroup-shared operand tiles (round 6).
// At molecule-batch sizes (M = 512) the tiling above wins: a launch has 8 ring slots of work per workgroup to hide its operand fetch
// behind, and splitting K over workgroups needs a combine launch that costs more than it saves (tools/probe/dense_lds_probe.hip,
// profiles/r06_dense_lds_probe.md: 13.8 + 2.8 us against 16.8).  From ~200 tiles on there is no split and the same design is 1.4-1.5 x
// the per-wave-operand kernel (M = 2048, K = N = 1024: 62 -> 43 us): a 64 x 128 macro-tile per 4-wave workgroup, both operands staged
// ONCE per workgroup by LDS-DMA into a ring of 32-k slots (24 KB each), each wave a 32 x 64 register tile (8 accumulators per 6
// fragment reads).  LDS image of a slot: row rho (0..63 the X rows, 64..191 the W rows) is 128 B = 8 pieces of 16 B (4 k each);
// logical piece lp sits at position lp ^ ((rho >> 1) & 7), so the sixteen lanes of every ds_read_b128 lane group touch sixteen
// different 16-byte bank groups (SQ_LDS_BANK_CONFLICT = 0).  The W rows are PERMUTED on the way in -- LDS row 64 + 64 c + 16 u + n
// holds W row j0 + 64 c + 4 n + u -- so that MFMA tile u of a wave covers the columns {4 n + u} and a lane's four accumulators of a
// row are four consecutive columns: bias, relu(dropout(.)) and the 16-byte stores go straight from registers, as in dense_tile.
// XCD x (workgroups b with b % 8 == x under round-robin dealing; speed only) takes the x-th contiguous eighth of the tiles, column
// tile major: the workgroups of an XCD share their W rows in its L2.  Same Philox stream as dense_tile's epilogue.
constexpr int kDtM = 64, kDtN = 128, kDtK = 32, kDtSlots = 4, kDtThreads = 256;
constexpr int kDtSlotFloats = (kDtM + kDtN) * kDtK;          // 24 KB
constexpr int kDtPieces = (kDtM + kDtN) / 8;                 // 1-KiB pieces per slot (8 rows x 128 B each): 24 = 6 per wave
constexpr int kDtLdsBytes = kDtSlots * kDtSlotFloats * 4;    // 96 KB: one workgroup per CU
constexpr int kDtMinTiles = 192;
template <int HA>
__global__ __launch_bounds__(kDtThreads) void k_dense_fwd_tiles(const DenseArgs T) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, l = tid & 63, n = l & 15, g = l >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int total = T.tiles_i * T.tiles_j, per_x = (total + 7) / 8;
    const int bx = (int)blockIdx.x & 7, bi = (int)blockIdx.x >> 3, t = bx * per_x + bi;
    if (bi >= per_x || t >= total) return;
    const int tn = t / T.tiles_i, tm = t - tn * T.tiles_i;
    const int i0 = tm * kDtM, j0 = tn * kDtN;
    const int M = T.I, N = T.J, K = T.R, lda = T.lda, ldb = T.ldb;
    const int nk = K / kDtK;                                 // K % 32 == 0 (host)
    const int tr = wv & 1, tc = wv >> 1;                     // this wave's 32 x 64 sub-tile
    const glb_f* Xb = G(T.A);
    const glb_f* Wb = G(T.Bsrc);
    auto issue = [&](int it) {
        float* slot = smem + (it % kDtSlots) * kDtSlotFloats;
        const int k0 = it * kDtK;
#pragma unroll
        for (int q = 0; q < kDtPieces / 4; ++q) {
            const int piece = wv + 4 * q;                    // wave-uniform
            const int rho = piece * 8 + (l >> 3);
            const int lp = (l & 7) ^ ((rho >> 1) & 7);
            const glb_f* src;
            if (piece < kDtM / 8) src = Xb + ((unsigned)min(i0 + rho, M - 1) * lda + k0 + 4 * lp);
            else {
                const int r = rho - kDtM, c = r >> 6, u = (r >> 4) & 3, nn = r & 15;
                src = Wb + ((unsigned)min(j0 + 64 * c + 4 * nn + u, N - 1) * ldb + k0 + 4 * lp);
            }
            __builtin_amdgcn_global_load_lds((const FN_GLB void*)src, (FN_LDS void*)(slot + piece * 256), 16, 0, 0);
        }
    };
    f32x4 acc[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < kDtSlots - 1; ++it) if (it < nk) issue(it);
    for (int it = 0; it < nk; ++it) {
        // slot `it` has landed for this wave once at most the pieces of the kDtSlots - 2 younger slots are outstanding; the barrier then
        // says so for every wave, and that everybody is done with the slot the next issue overwrites
        if (it + kDtSlots - 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kDtSlots - 2) * (kDtPieces / 4)) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (it + kDtSlots - 1 < nk) issue(it + kDtSlots - 1);
        const lds_f* slot = (const lds_f*)(smem + (it % kDtSlots) * kDtSlotFloats);
        auto frag = [&](int rho, int kk) { return *reinterpret_cast<const FN_LDS f32x4*>(slot + rho * 32 + 4 * ((4 * kk + g) ^ ((rho >> 1) & 7))); };
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 a[2], bw[4];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) a[t2] = frag(32 * tr + 16 * t2 + n, kk);
#pragma unroll
            for (int u = 0; u < 4; ++u) bw[u] = frag(kDtM + 64 * tc + 16 * u + n, kk);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int u = 0; u < 4; ++u) DN_MFMA(acc[4 * t2 + u], a[t2][q], bw[u][q]);
        }
    }
    // acc[4 t + u][e] = (row 32 tr + 16 t + 4 g + e, column 64 tc + 4 n + u) of the tile
    const bool act_on = HA < 0 && T.act.y != nullptr;
    const float p = T.act.p, ik = p < 1.f ? 1.f / (1.f - p) : 0.f;
    const uint64_t rng = act_on && p > 0.f ? T.act.offset + (T.act.offset_dev ? *T.act.offset_dev : 0) : 0;
    HactRun hr{};
    if constexpr (HA >= 0) hr = hact_run(T.hact, HA);
    glb_f* OUT = G(T.OUT);
    const int gj = j0 + 64 * tc + 4 * n;
    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T.bias && gj < N) bb = ld4(G(T.bias) + gj);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int gi = i0 + 32 * tr + 16 * t2 + 4 * g + e;
            if (gi >= M || gj >= N) continue;                // N % 4 == 0
            float4 v = make_float4(acc[4 * t2][e] + bb.x, acc[4 * t2 + 1][e] + bb.y, acc[4 * t2 + 2][e] + bb.z, acc[4 * t2 + 3][e] + bb.w);
            if (act_on) {
                if (p > 0.f) {
                    const uint4 rnd = philox4x32(rng + ((uint64_t)gi * N + gj) / 4, T.act.seed);
                    v.x *= keep_scale(rnd.x, p, ik);  v.y *= keep_scale(rnd.y, p, ik);
                    v.z *= keep_scale(rnd.z, p, ik);  v.w *= keep_scale(rnd.w, p, ik);
                }
                if (T.act.relu) { v.x = fmaxf(v.x, 0.f);  v.y = fmaxf(v.y, 0.f);  v.z = fmaxf(v.z, 0.f);  v.w = fmaxf(v.w, 0.f); }
            }
            if constexpr (HA >= 0) {
                float4 u;
                v = hact_fwd4<HA>(T.hact, hr, v, (uint64_t)gi * N + gj, u);
                st4(G(T.hact.pre) + ((size_t)gi * N + gj), u);
            }
            st4(OUT + ((size_t)gi * N + gj), v);
        }
}

template <int HA>
__global__ __launch_bounds__(kDnThreads, 4) void k_dense_fwd(const DenseArgs T, const int narrow) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (narrow) dense_tile<DN_FWD, 2, HA>(T, (int)blockIdx.x, (lds_f*)smem);
    else dense_tile<DN_FWD, 4, HA>(T, (int)blockIdx.x, (lds_f*)smem);
}
// What the fused last Linear + loss launch (k_small_linear_loss) leaves for "the next launch": dW[C,K] = g^T x, db[C] = colsum(g) and the
// loss value from its per-block partials.  These blocks ride at the end of the first k_dense_bwd launch of the head's backward.
// A block owns 16 columns k for all rows (4 float4 columns x 128 row lanes, U rows per trip in flight), sums its 128 partial rows
// through LDS in two fixed-order stages; one more block takes db (a wave per class) and the loss.
struct SmallDw {
    const float *g, *x;        // [M,C], [M,K]
    float *dW, *db;            // [C,K], [C]
    const float* loss_part;    // [n_part]
    float* loss;               // [1]
    int n_part, M, K, C, first_block;     // first_block < 0: no such blocks
};
template <int CM>
__device__ __forceinline__ void small_dw_cols(const SmallDw& S, int vb, lds_f* smem) {
    const int c4 = threadIdx.x & 3, rl = threadIdx.x >> 2;            // 4 float4 columns x 128 row lanes
    const int col = vb * 16 + c4 * 4, K = S.K, C = S.C, M = S.M;
    const bool live = col < K;
    float4 acc[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
        constexpr int U = CM > 4 ? 2 : 4;
        for (int m0 = rl; m0 < M; m0 += U * 128) {
            float4 xv[U];
            float gv[U][CM];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = m0 + 128 * u < M ? m0 + 128 * u : m0;
                xv[u] = ld4(S.x + (size_t)m * K + col);
#pragma unroll
                for (int c = 0; c < CM; ++c) gv[u][c] = c < C ? S.g[(size_t)m * C + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (m0 + 128 * u >= M) continue;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    acc[c].x += gv[u][c] * xv[u].x; acc[c].y += gv[u][c] * xv[u].y;
                    acc[c].z += gv[u][c] * xv[u].z; acc[c].w += gv[u][c] * xv[u].w;
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        if (c < C) {                                                  // uniform
            st4s(smem + (rl * 4 + c4) * 4, acc[c]);
            __syncthreads();
            if (rl < 8) {                                             // stage 1: row lanes rl, rl + 8, ... (16 each)
                float4 t = ld4s(smem + (rl * 4 + c4) * 4);
                for (int q = 1; q < 16; ++q) { const float4 u = ld4s(smem + ((rl + 8 * q) * 4 + c4) * 4); t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
                st4s(smem + (128 * 4 + rl * 4 + c4) * 4, t);
            }
            __syncthreads();
            if (rl == 0 && live) {                                    // stage 2: the eight partial sums in order
                float4 t = ld4s(smem + (128 * 4 + c4) * 4);
                for (int q = 1; q < 8; ++q) { const float4 u = ld4s(smem + (128 * 4 + q * 4 + c4) * 4); t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
                st4(S.dW + (size_t)c * K + col, t);
            }
            __syncthreads();
        }
    }
}
__device__ __forceinline__ void small_dw_block(const SmallDw& S, int vb, lds_f* smem) {
    const int nk = (S.K + 15) / 16;
    if (vb < nk) {
        if (S.C <= 1) small_dw_cols<1>(S, vb, smem);
        else if (S.C <= 4) small_dw_cols<4>(S, vb, smem);
        else small_dw_cols<FN_SMALL_LINEAR_MAX>(S, vb, smem);
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int c = wv; c < S.C; c += kDnWaves) {                        // bias gradient: one wave per class, fixed order
        float t = 0.f;
        for (int m = lane; m < S.M; m += 64) t += S.g[(size_t)m * S.C + c];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) S.db[c] = t;
    }
    if (wv == kDnWaves - 1 && S.loss) {                               // the loss: the launch before left one partial per block
        float t = 0.f;
        for (int i = lane; i < S.n_part; i += 64) t += S.loss_part[i];
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
        if (lane == 0) S.loss[0] = t;
    }
}

// the two gradient products of a layer in one launch: blocks [0, b.first_block) the weight gradient, the rest the input gradient
// (and, behind those, the riders of the fused last Linear: SmallDw)
// (HA >= 0: the input gradient goes through the layer below's activation kind, head_act.inc)
template <int HA>
__global__ __launch_bounds__(kDnThreads, 4) void k_dense_bwd(const DensePair P, const SmallDw S) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = (int)blockIdx.x;
    if (S.first_block >= 0 && b >= S.first_block) { small_dw_block(S, b - S.first_block, (lds_f*)smem);  return; }
    if (b < P.b.first_block) { if (P.a_narrow) dense_dw_narrow(P.a, b, (lds_f*)smem); else dense_tile<DN_DW>(P.a, b, (lds_f*)smem); }
    else if (P.b_narrow) dense_tile<DN_DX, 2, HA>(P.b, b - P.b.first_block, (lds_f*)smem);
    else dense_tile<DN_DX, 4, HA>(P.b, b - P.b.first_block, (lds_f*)smem);
}
