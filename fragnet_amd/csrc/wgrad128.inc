// Weight-gradient partial products dW[128 o][128 k] = sum_rows dY[r][o] X[r][k] of the K = 128 projections, direct form
// (included into the anonymous namespace of param_grads.hip; WgradTask / WgradTasks: fn_internal.h; FN_TUNE_WGRAD_DIRECT).
//
// Both operands run ACROSS the reduction index (a row of dY / X is contiguous in o / k), so -- as in csrc/dense_head.inc --
// lane (n, g) of v_mfma_f32_16x16x4_f32 takes the four columns 4n .. 4n+3 of row r0 + g of each operand as one 16-byte
// piece, and component q (q') feeds the accumulator of the output rows {4n + q} (columns {4n' + q'}): 16 MFMAs per two
// 16-byte LDS reads (k_linear128_wgrad reads its staged operands back one scalar per MFMA).  A workgroup = 8 waves = the four 64 x 64 tiles of the
// 128 x 128 result x two interleaved halves of the block's rows; the halves are added through LDS and the block writes one
// partial in plain [o][k] layout (+ the column sums of dY = the bias-gradient partial); the deferred reduction adds the
// blocks (RT_WGRAD, cls 4).
constexpr int kWdSlotRows = 64;                            // rows of a ring slot
constexpr int kWdSlotFloats = 2 * kWdSlotRows * 128;       // dY rows | X rows: 64 KB
constexpr int kWdTile = 4 * 64 * 64 + 128;                 // LDS floats of one hand-over slot: four 64x64 tiles + 128 column sums
constexpr int kWdPartWidth = 128 * 128 + 128;              // == the partial width of k_linear128_wgrad<4, 2>
template <int NS> constexpr int wd_threads() { return 256 * NS; }
template <int NS> constexpr int wd_lds_bytes() { return 2 * kWdSlotFloats * 4; }      // two ring slots (the hand-over reuses them)
static_assert(kWdTile <= 2 * kWdSlotFloats, "the hand-over slots fit the ring");

// Round 3: the rows go global -> LDS by LDS-DMA, ONCE per workgroup, and the waves read their operand pieces from LDS.  Before,
// every wave loaded its own pieces from global memory: each row was fetched by two waves of each half (the 2 x 2 tiles share
// dY / X column halves), 32 B per clock and CU through the vector-memory path for the 16 MFMAs of a step -- exactly the measured
// ceiling of that path for L2 hits, which is why the matrix pipe sat at 58 %.  Two 64-row slots: slot k+1 is in flight while
// slot k is multiplied (the barrier at a slot boundary drains the DMA, hipcc's __syncthreads waits vmcnt(0)).
template <int NS>
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
    // 64 pieces of 1 KiB per slot (two rows each): pieces 0..31 the dY rows, 32..63 the X rows; NW waves take them round robin
    auto issue = [&](int slot, int buf) {
#pragma unroll
        for (int i = 0; i < 64 / NW; ++i) {
            const int piece = wv + NW * i, op = piece >> 5, pr = piece & 31;
            const int row = min(slot * kWdSlotRows + 2 * pr + (l >> 5), rows - 1);          // rows past the end: any valid row (masked below)
            const float* src = (op ? t.X : t.dY) + (size_t)(m_begin + row) * 128 + (l & 31) * 4;
            dma_to_lds<16>(src, smem_raw + buf * kWdSlotFloats + op * (kWdSlotRows * 128) + pr * 256);
        }
    };
    if (nslots > 0) issue(0, 0);
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
            const float av[4] = {fa.x, fa.y, fa.z, fa.w};
            dbacc.x += av[0];  dbacc.y += av[1];  dbacc.z += av[2];  dbacc.w += av[3];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                DN_MFMA(acc[4 * q + 0], av[q], fb.x);  DN_MFMA(acc[4 * q + 1], av[q], fb.y);
                DN_MFMA(acc[4 * q + 2], av[q], fb.z);  DN_MFMA(acc[4 * q + 3], av[q], fb.w);
            }
        }
    }
    __syncthreads();                                        // the ring is free: the hand-over below reuses it
    // column sums of dY over this lane group's rows -> over the four groups (fixed order)
    dbacc.x += __shfl_xor(dbacc.x, 16);  dbacc.y += __shfl_xor(dbacc.y, 16);  dbacc.z += __shfl_xor(dbacc.z, 16);  dbacc.w += __shfl_xor(dbacc.w, 16);
    dbacc.x += __shfl_xor(dbacc.x, 32);  dbacc.y += __shfl_xor(dbacc.y, 32);  dbacc.z += __shfl_xor(dbacc.z, 32);  dbacc.w += __shfl_xor(dbacc.w, 32);
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
        }
        if (act > 1) __syncthreads();                       // the slots are rewritten in the next round
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
                st4(pw + (size_t)(64 * ta + row) * 128 + 64 * tb + 4 * n, v);
            }
        if (tb == 0 && l < 16) {
            const float4 o = ld4s(dbp + 64 * ta + 4 * n);
            float4 v = make_float4(dbacc.x + o.x, dbacc.y + o.y, dbacc.z + o.z, dbacc.w + o.w);
            st4(pw + 128 * 128 + 64 * ta + 4 * n, v);
        }
    }
}

template <int NS>
__global__ __launch_bounds__(256 * NS, 2) void k_wgrad128_multi(const WgradTasks T) {
    extern __shared__ __attribute__((aligned(16))) float smem_raw[];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    wgrad128_block<NS>(T.t[ti], (int)blockIdx.x - T.t[ti].first, smem_raw);
}
