// Weight-gradient partial products dW[128 o][128 k] = sum_rows dY[r][o] X[r][k] of the K = 128 projections, direct form
// (included into the anonymous namespace of encoder.hip after WgradTasks; FN_TUNE_WGRAD_DIRECT).
//
// Both operands run ACROSS the reduction index (a row of dY / X is contiguous in o / k), so -- as in csrc/dense_head.inc --
// lane (n, g) of v_mfma_f32_16x16x4_f32 takes the four columns 4n .. 4n+3 of row r0 + g of each operand as one 16-byte
// piece, and component q (q') feeds the accumulator of the output rows {4n + q} (columns {4n' + q'}): 16 MFMAs per two
// 16-byte LDS reads (k_linear128_wgrad reads its staged operands back one scalar per MFMA).  A workgroup = 8 waves = the four 64 x 64 tiles of the
// 128 x 128 result x two interleaved halves of the block's rows; the halves are added through LDS and the block writes one
// partial in plain [o][k] layout (+ the column sums of dY = the bias-gradient partial); the deferred reduction adds the
// blocks (RT_WGRAD, cls 4).
#ifndef FN_WG_ENDFIX
#define FN_WG_ENDFIX 1      // 1: the term is added to the block's partial at the END (dW += a_dst[c] U[h(c)], db += a_dst[c] S[h(c)]: the product is
#endif                      //    linear and U is accumulated anyway), the waves of dY columns 64..127 then do nothing extra per step; 0: on the dY operand
constexpr int kWdSlotRows = 64;                            // rows of a ring slot
constexpr int kWdSlotFloats = 2 * kWdSlotRows * 128;       // dY rows | X rows: 64 KB
constexpr int kWdU = 4 * 128 + 16;                         // the deferred term's side product: U[4][128] + S[4] (padded)
constexpr int kWdTile = 4 * 64 * 64 + 128 + kWdU;          // LDS floats of one hand-over slot: four 64x64 tiles + 128 column sums + U, S
constexpr int kWdPartWidth = 128 * 128 + 128;              // == the partial width of k_linear128_wgrad<4, 2>
constexpr int kWdUWidth = 4 * 128 + 4;                     // floats per block in WgradTask::upart (K = 128): U[h][k], then S[h]
constexpr int kWdGsd = 2 * kWdSlotRows * 4;                // behind the ring: the slots' g_s_dst rows ([64][4] each; deferred term only)
template <int NS> constexpr int wd_threads() { return 256 * NS; }
template <int NS> constexpr int wd_lds_bytes() { return (2 * kWdSlotFloats + kWdGsd) * 4; }      // two ring slots (the hand-over reuses them) + g_s_dst rows
static_assert(kWdTile <= 2 * kWdSlotFloats, "the hand-over slots fit the ring");

// Round 3: the rows go global -> LDS by LDS-DMA, ONCE per workgroup, and the waves read their operand pieces from LDS.  Before,
// every wave loaded its own pieces from global memory: each row was fetched by two waves of each half (the 2 x 2 tiles share
// dY / X column halves), 32 B per clock and CU through the vector-memory path for the 16 MFMAs of a step -- exactly the measured
// ceiling of that path for L2 hits, which is why the matrix pipe sat at 58 %.  Two 64-row slots: slot k+1 is in flight while
// slot k is multiplied (the barrier at a slot boundary drains the DMA, hipcc's __syncthreads waits vmcnt(0)).
// DF (the deferred term) and UJ (this wave also accumulates the side product U: the waves of dY columns 0..63) are COMPILE-TIME
// variants of the slot loop: as run-time branches inside it they cost the plain products 14 us per launch (65.6 -> 79.6 us: every
// step became a basic block of its own and the LDS reads no longer overlapped the previous step's MFMAs).
template <int NS, bool DF>
__device__ __forceinline__ void wgrad128_block(const WgradTask& t, int bid, float* smem_raw) {
    lds_f* smem = (lds_f*)smem_raw;
    constexpr int NW = 4 * NS;                              // waves of the workgroup
    const int tid = threadIdx.x, l = tid & 63, n = l & 15, g = l >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = wv & 3, ta = tile >> 1, tb = tile & 1, half = wv >> 2;
    const int64_t M = t.n_real && *t.n_real < t.M ? (int64_t)*t.n_real : t.M;      // rows behind it: padding, zero gradient rows
    const int64_t m_begin = (int64_t)bid * t.rpb;
    const int64_t m_end = m_begin + t.rpb < M ? m_begin + t.rpb : M;
    const int rows = m_end > m_begin ? (int)(m_end - m_begin) : 0;
    const int nslots = (rows + kWdSlotRows - 1) / kWdSlotRows;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4 acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float4 dbacc = zero4;
    // The deferred form of the one-pass attention backward (gat_bwd_one.inc, DF): the dY rows are the level's g_h WITHOUT the term
    // g_s_dst[row] a_dst.  It is added here, to the operand piece as it leaves LDS (the piece's four columns belong to one head: one
    // scalar x four constants), so dW and db come out exact; and the waves that own the tiles of dY columns 0..63 also accumulate the
    // side product U[h][k] = sum_rows g_s_dst[row, h] X[row, k] and S[h] = sum_rows g_s_dst[row, h] (sixteen vector FMAs beside sixteen
    // MFMAs), from which the deferred reduction forms dL/da_dst = W U^T + b S without anybody reading the projected rows h again.
    constexpr bool df = DF;                                // (four heads: the engine's condition for the deferred form)
    const int hA = (64 * ta + 4 * n) >> 5;
    const float4 a4 = df ? ld4(t.a_dst + hA * t.att_w + ((64 * ta + 4 * n) & 31)) : zero4;
    float4 uacc[4] = {zero4, zero4, zero4, zero4};
    float4 sacc = zero4;
    // 64 pieces of 1 KiB per slot (two rows each): pieces 0..31 the dY rows, 32..63 the X rows; NW waves take them round robin
    auto issue = [&](int slot, int buf) {
#pragma unroll
        for (int i = 0; i < 64 / NW; ++i) {
            const int piece = wv + NW * i, op = piece >> 5, pr = piece & 31;
            const int row = min(slot * kWdSlotRows + 2 * pr + (l >> 5), rows - 1);          // rows past the end: any valid row (masked below)
            const float* src = (op ? t.X : t.dY) + (size_t)(m_begin + row) * 128 + (l & 31) * 4;
            dma_to_lds<16>(src, smem_raw + buf * kWdSlotFloats + op * (kWdSlotRows * 128) + pr * 256);
        }
        if (DF && wv == 0) {                                // the slot's 64 g_s_dst rows (16 bytes each): one more piece
            const int row = min(slot * kWdSlotRows + l, rows - 1);
            dma_to_lds<16>(t.gsd + (size_t)(m_begin + row) * 4, smem_raw + 2 * kWdSlotFloats + buf * (kWdSlotRows * 4));
        }
    };
    if (nslots > 0) issue(0, 0);
    auto slots = [&](auto uj_tag) {
        constexpr bool UJ = decltype(uj_tag)::value;
        for (int slot = 0; slot < nslots; ++slot) {
            const int buf = slot & 1;
            __syncthreads();                                    // this slot has landed; everybody is done with the other one
            if (slot + 1 < nslots) issue(slot + 1, buf ^ 1);
            const lds_f* A = smem + buf * kWdSlotFloats + 64 * ta + 4 * n;
            const lds_f* B = smem + buf * kWdSlotFloats + kWdSlotRows * 128 + 64 * tb + 4 * n;
#pragma unroll
            for (int st = 0; st < kWdSlotRows / 4 / NS; ++st) {
                const int r = 4 * (half + NS * st) + g;         // the halves take alternate 4-row steps
                const bool ok = slot * kWdSlotRows + r < rows;
                float4 fa = ld4s(A + r * 128), fb = ld4s(B + r * 128);
                if (!ok) { fa = zero4;  fb = zero4; }
                if constexpr (DF && (UJ || !FN_WG_ENDFIX)) {
                    float4 gq = ld4s(smem + 2 * kWdSlotFloats + buf * (kWdSlotRows * 4) + r * 4);
                    if (!ok) gq = zero4;
                    const float gh = hA == 0 ? gq.x : hA == 1 ? gq.y : hA == 2 ? gq.z : gq.w;
                    if (!FN_WG_ENDFIX) { fa.x = fmaf(gh, a4.x, fa.x);  fa.y = fmaf(gh, a4.y, fa.y);  fa.z = fmaf(gh, a4.z, fa.z);  fa.w = fmaf(gh, a4.w, fa.w); }
                    if constexpr (UJ) {
                        fma4(uacc[0], gq.x, fb);  fma4(uacc[1], gq.y, fb);  fma4(uacc[2], gq.z, fb);  fma4(uacc[3], gq.w, fb);
                        sacc.x += gq.x;  sacc.y += gq.y;  sacc.z += gq.z;  sacc.w += gq.w;
                    }
                }
                const float av[4] = {fa.x, fa.y, fa.z, fa.w};
                dbacc.x += av[0];  dbacc.y += av[1];  dbacc.z += av[2];  dbacc.w += av[3];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    DN_MFMA(acc[4 * q + 0], av[q], fb.x);  DN_MFMA(acc[4 * q + 1], av[q], fb.y);
                    DN_MFMA(acc[4 * q + 2], av[q], fb.z);  DN_MFMA(acc[4 * q + 3], av[q], fb.w);
                }
            }
        }
    };
    if (DF && ta == 0) slots(std::true_type{});
    else slots(std::false_type{});
    __syncthreads();                                        // the ring is free: the hand-over below reuses it
    // column sums of dY over this lane group's rows -> over the four groups (fixed order)
    dbacc.x += __shfl_xor(dbacc.x, 16);  dbacc.y += __shfl_xor(dbacc.y, 16);  dbacc.z += __shfl_xor(dbacc.z, 16);  dbacc.w += __shfl_xor(dbacc.w, 16);
    dbacc.x += __shfl_xor(dbacc.x, 32);  dbacc.y += __shfl_xor(dbacc.y, 32);  dbacc.z += __shfl_xor(dbacc.z, 32);  dbacc.w += __shfl_xor(dbacc.w, 32);
    const bool uw = df && ta == 0;                          // this wave holds a column half of U (and, tb == 0, S)
    if (uw) {
        auto red4 = [](float4& v) {
            v.x += __shfl_xor(v.x, 16);  v.y += __shfl_xor(v.y, 16);  v.z += __shfl_xor(v.z, 16);  v.w += __shfl_xor(v.w, 16);
            v.x += __shfl_xor(v.x, 32);  v.y += __shfl_xor(v.y, 32);  v.z += __shfl_xor(v.z, 32);  v.w += __shfl_xor(v.w, 32);
        };
#pragma unroll
        for (int hh = 0; hh < 4; ++hh) red4(uacc[hh]);
        red4(sacc);
    }
    // the upper slices hand their tiles to the lower ones through LDS, pairwise (slice h + act -> slice h), in a fixed order;
    // acc[q][q'][e] is (row 4(4g + e) + q, columns 4n + q')
#pragma unroll
    for (int act = NS / 2; act >= 1; act >>= 1) {
        if (half >= act && half < 2 * act) {
            lds_f* part = smem + (half - act) * kWdTile + tile * 4096;
            lds_f* dbp = smem + (half - act) * kWdTile + 4 * 4096;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    st4s(part + (4 * (4 * g + e) + q) * 64 + 4 * n, make_float4(acc[4 * q][e], acc[4 * q + 1][e], acc[4 * q + 2][e], acc[4 * q + 3][e]));
            if (tb == 0 && l < 16) st4s(dbp + 64 * ta + 4 * n, dbacc);
            if (uw && l < 16) {
                lds_f* up = smem + (half - act) * kWdTile + 4 * 4096 + 128;
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) st4s(up + hh * 128 + 64 * tb + 4 * n, uacc[hh]);
                if (tb == 0 && l == 0) st4s(up + 512, sacc);
            }
        }
        __syncthreads();
        if (half < act && act > 1) {                        // fold and keep going
            const lds_f* part = smem + half * kWdTile + tile * 4096;
            const lds_f* dbp = smem + half * kWdTile + 4 * 4096;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float4 o = ld4s(part + (4 * (4 * g + e) + q) * 64 + 4 * n);
                    acc[4 * q][e] += o.x;  acc[4 * q + 1][e] += o.y;  acc[4 * q + 2][e] += o.z;  acc[4 * q + 3][e] += o.w;
                }
            if (tb == 0 && l < 16) {
                const float4 o = ld4s(dbp + 64 * ta + 4 * n);
                dbacc.x += o.x;  dbacc.y += o.y;  dbacc.z += o.z;  dbacc.w += o.w;
            }
            if (uw && l < 16) {
                const lds_f* up = smem + half * kWdTile + 4 * 4096 + 128;
#pragma unroll
                for (int hh = 0; hh < 4; ++hh) {
                    const float4 o = ld4s(up + hh * 128 + 64 * tb + 4 * n);
                    uacc[hh].x += o.x;  uacc[hh].y += o.y;  uacc[hh].z += o.z;  uacc[hh].w += o.w;
                }
                if (tb == 0 && l == 0) { const float4 o = ld4s(up + 512);  sacc.x += o.x;  sacc.y += o.y;  sacc.z += o.z;  sacc.w += o.w; }
            }
        }
        if (act > 1) __syncthreads();                       // the slots are rewritten in the next round
    }
    float4 ufix = zero4;        // end fix: U[head of this lane's output rows][this lane's four columns]
    float sfix[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (DF && FN_WG_ENDFIX && NS == 2) {
        lds_f* uT = smem + kWdTile;                         // the block's complete U [4][128], then S [4]
        if (uw && half == 0 && l < 16) {
            const lds_f* up = smem + 4 * 4096 + 128;
#pragma unroll
            for (int hh = 0; hh < 4; ++hh) {
                const float4 o = ld4s(up + hh * 128 + 64 * tb + 4 * n);
                uacc[hh] = make_float4(uacc[hh].x + o.x, uacc[hh].y + o.y, uacc[hh].z + o.z, uacc[hh].w + o.w);
                st4s(uT + hh * 128 + 64 * tb + 4 * n, uacc[hh]);
            }
            if (tb == 0 && l == 0) {
                const float4 o = ld4s(up + 512);
                sacc = make_float4(sacc.x + o.x, sacc.y + o.y, sacc.z + o.z, sacc.w + o.w);
                st4s(uT + 512, sacc);
            }
        }
        __syncthreads();
        ufix = ld4s(uT + (2 * ta + (g >> 1)) * 128 + 64 * tb + 4 * n);          // rows 4 (4 g + e) + q of the tile: head 2 ta + (g >> 1)
        const float4 s4 = ld4s(uT + 512);
        sfix[0] = s4.x;  sfix[1] = s4.y;  sfix[2] = s4.z;  sfix[3] = s4.w;
    }
    if (half == 0) {
        const lds_f* part = smem + tile * 4096;
        const lds_f* dbp = smem + 4 * 4096;
        glb_f* pw = G(t.part) + (size_t)bid * kWdPartWidth;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = 4 * (4 * g + e) + q;
                const float4 o = ld4s(part + row * 64 + 4 * n);
                float4 v = make_float4(acc[4 * q][e] + o.x, acc[4 * q + 1][e] + o.y, acc[4 * q + 2][e] + o.z, acc[4 * q + 3][e] + o.w);
                if constexpr (DF && FN_WG_ENDFIX && NS == 2) fma4(v, t.a_dst[(2 * ta + (g >> 1)) * t.att_w + (row & 31)], ufix);
                st4(pw + (size_t)(64 * ta + row) * 128 + 64 * tb + 4 * n, v);
            }
        if (tb == 0 && l < 16) {
            const float4 o = ld4s(dbp + 64 * ta + 4 * n);
            float4 v = make_float4(dbacc.x + o.x, dbacc.y + o.y, dbacc.z + o.z, dbacc.w + o.w);
            if constexpr (DF && FN_WG_ENDFIX && NS == 2) {
                const int hb = 2 * ta + (n >> 3);                        // head of the columns 64 ta + 4 n ..
                const float4 ad = ld4(t.a_dst + hb * t.att_w + ((4 * n) & 31));
                const float sh = hb == 0 ? sfix[0] : hb == 1 ? sfix[1] : hb == 2 ? sfix[2] : sfix[3];
                fma4(v, sh, ad);
            }
            st4(pw + 128 * 128 + 64 * ta + 4 * n, v);
        }
        if (uw && l < 16) {
            const lds_f* up = smem + 4 * 4096 + 128;
            glb_f* upw = G(t.upart) + (size_t)bid * kWdUWidth;
            const bool summed = DF && FN_WG_ENDFIX && NS == 2;       // (the end fix already added the other half's share)
#pragma unroll
            for (int hh = 0; hh < 4; ++hh) {
                const float4 o = summed ? zero4 : ld4s(up + hh * 128 + 64 * tb + 4 * n);
                st4(upw + hh * 128 + 64 * tb + 4 * n, make_float4(uacc[hh].x + o.x, uacc[hh].y + o.y, uacc[hh].z + o.z, uacc[hh].w + o.w));
            }
            if (tb == 0 && l == 0) {
                const float4 o = summed ? zero4 : ld4s(up + 512);
                st4(upw + 512, make_float4(sacc.x + o.x, sacc.y + o.y, sacc.z + o.z, sacc.w + o.w));
            }
        }
    }
}

template <int NS>
__global__ __launch_bounds__(256 * NS, 2) void k_wgrad128_multi(const WgradTasks T) {
    extern __shared__ __attribute__((aligned(16))) float smem_raw[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    if (T.t[ti].gsd) wgrad128_block<NS, true>(T.t[ti], (int)blockIdx.x - T.t[ti].first, smem_raw);
    else wgrad128_block<NS, false>(T.t[ti], (int)blockIdx.x - T.t[ti].first, smem_raw);
}
