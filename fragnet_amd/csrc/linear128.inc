// linear128.inc -- the fp32-MFMA [M,K] x [K,128] tile body and its fused epilogues (included, inside the anonymous namespace, by
// fragnet_hip.hip -- the projection launches --, by encoder.hip -- k_lin_rd_cu, the input-gradient products beside the edge term's backward --
// and by gat_fwd_lin.hip, whose launches carry projection tiles beside an attention pass).  Templates only.  Argument blocks: fn_internal.h.
// =====================================================================================
// Projection GEMMs on the fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 FMA chains, so the 1e-4
// parity budget is untouched).  All three node projections have N = 128 outputs and K <= 168 inputs:
//   forward    Y[M,128]  = X[M,K]   * Bt[K,128] + bias      (Bt = W^T, transposed once per step)
//   input grad dX[M,128] = dY[M,128] * W[128,128]            (same kernel, Bt = W as stored, no bias)
//   weight grad dW[128,K] = dY^T X, db = colsum(dY)           (split over row chunks, deterministic 2-stage sum)
// =====================================================================================
struct __attribute__((packed, aligned(4))) f32x4_u4 { float v[4]; };      // 16 bytes at a 4-byte-aligned address
constexpr int kBtLd = 144;     // LDS leading dimension of the [K][128] operand: 144 % 32 == 16
constexpr int kLinLd = 64;     // k_linear128's operand tile [K][64 columns], unpadded: a lane reads 4 consecutive columns (ds_read_b128) and the
                               // 16-lane groups of that instruction then cover all 64 banks exactly once (rows 4 apart share the bank alignment)

// A block = 8 waves = 64 rows x 128 columns: wave w owns rows 16*(w&3).. and columns 64*(w>>2).. (4 accumulator
// tiles), so two waves share every SIMD and one wave's LDS reads hide under the other's MFMAs.  Bt is staged in
// LDS once per block; blocks loop over row tiles.  The MFMA k index is "blocked": lane group kq supplies
// k = kq*KQ + s at step s, so a lane's A operands are KQ consecutive floats of one row, loaded with 16-byte loads
// straight from global memory (no LDS round trip for X) and prefetched one tile ahead.  The result tile goes
// through LDS so that every lane stores whole 16-byte pieces of a row (scattered 4-byte stores cost 4 us a tile).
constexpr int kLinWaves = 4, kLinThreads = 64 * kLinWaves, kLinRows = 16 * kLinWaves;   // a block: kLinRows rows x 64 columns
constexpr int kLinOutLd = 68;      // LDS leading dimension of a wave's 16 x 64 result tile
using fni::NodeScalarEpi;
// VEC (K == 4*KQ, KQ % 4 == 0): lane (i, kq) owns the k's {16 s + 4 kq + c}: one wave-instruction then reads 64
// contiguous bytes of each of its 16 rows (a blocked split, k = kq*KQ + .., made every lane touch its own 128-byte
// line and re-fetched each line eight times through a thrashing L1).  The B rows in LDS are indexed to match.
// optional epilogue term of an input-gradient product (RA instances): Y[row, :] += sum_h z[row, h] * a[h * lda + :], h < 4 -- the
// backward of the atom graph's edge term <new_bond[e], a[h, mid block]> lands on the bond rows without a pass of its own
using fni::RowAdd;
// optional epilogue of an input-gradient product (CU instances): the two node-local dots of the finished gradient row the one-pass
// attention backward needs (gat_bwd_one.inc): c[row, h] = scale <Y[row, head cols], out[row, head cols]> and
// u[row, h] = <Y[row, ...], out2[row, ...]> - c sigma[row, h].  out == null: the row reaches its level through relu(dropout(.))
// only, and the gate's saved output y (loaded for the gate anyway) stands in for it with scale = 1 - p.
constexpr int kCuRows = 4;        // rows of a lane's four whose epilogue operands are in flight together (CuEpi): all four.  Two at a time
                                  // fit four waves per SIMD only with spills: the launch measured 43-45 us against 34-36
using fni::CuEpi;
// POL: the output rows take the next-launch store policy (fn_internal.h).  The stand-alone operator kernel k_linear128 passes false: with
// the buffer store two of its instances (K <= 8, and K = 167 with the fused gate) would lose a wave per SIMD.
template <int KQ, bool VEC, bool PF, bool RA = false, bool CU = false, bool POL = true>
__device__ __forceinline__ void linear128_body(float* sBt, const float* __restrict__ X, int K, const float* __restrict__ Bt,
                                               const float* __restrict__ bias, float* __restrict__ Y, int64_t M,
                                               const fn_act_epilogue& mk, const NodeScalarEpi& ns, int bid, int nblk,
                                               const RowAdd& ra = RowAdd{nullptr, nullptr, 0},
                                               const CuEpi& cu = CuEpi{nullptr, nullptr, nullptr, nullptr, nullptr, 0},
                                               const int32_t* n_real = nullptr) {
    // A block is 4 waves = 64 rows x 64 COLUMNS (column half wc = bid & 1) and walks the row tiles bid>>1, += nblk>>1.
    // sBt: the [4*KQ][kLinLd] operand tile of this column half, staged ONCE; after that the block never synchronises
    // again: A rows live in registers (PF: the next tile's rows are requested before this tile's MFMA chain), and
    // with column-interleaved MFMA tiles (tile t = columns {4 i + t}) a lane's four accumulators of one row ARE a
    // float4 of four consecutive columns, so results, bias and fused epilogues go straight from registers to global
    // memory (16 lanes = 256 contiguous bytes of a row) — no LDS transpose, 33 KB per block, four blocks per CU whose
    // waves drift out of phase (in-phase staging / multiply / store rounds left the MFMA pipe 70 % idle, PMC).
    const uint64_t mk_base = mk.offset + ((mk.y && mk.p > 0.f && mk.offset_dev) ? *mk.offset_dev : 0);   // read once, not per tile
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 15, kq = lane >> 4;
    const int stride = nblk >> 1;
    int64_t tiles = (M + kLinRows - 1) / kLinRows;
    if (n_real) {                                            // padding rows of a static-shape batch: their tiles are skipped
        const int64_t live = ((int64_t)*n_real + kLinRows - 1) / kLinRows;
        tiles = live < tiles ? live : tiles;
    }
    // Which (row tile, column half) this block starts with.  The two halves of a row tile read the same 32 KB of A rows; workgroups
    // are dealt round-robin over the 8 XCDs, so neighbours b, b + 1 never share an L2 and the rows crossed the fabric twice
    // (PMC: the one-pass backward's product launch fetched 118 MB for 87 MB of operands).  Blocks b and b + 8 do share one: within
    // every group of 16 blocks the first eight take half 0 of eight tiles, the second eight half 1 of the same tiles.
#ifndef FN_LIN_PAIR_XCD
#define FN_LIN_PAIR_XCD 1
#endif
    int wc;
    int64_t tile;
    const int full = FN_LIN_PAIR_XCD ? (nblk >> 4) << 4 : 0;
    if (bid < full) { wc = (bid >> 3) & 1;  tile = (int64_t)(bid >> 4) * 8 + (bid & 7); }
    else { wc = (bid - full) & 1;  tile = (full >> 1) + ((bid - full) >> 1); }        // the last, incomplete group: neighbours
    // (Also giving XCD x the x-th CONTIGUOUS eighth of the row tiles -- the rows the same XCD gathers in the next launch's attention
    // pass -- measured slower: the attention launches did not change, i.e. nothing survives in an L2 across the kernel boundary, and
    // the product launches lost 2 us each with every XCD streaming one address range: 0.795-0.798 -> 0.806-0.809 ms per step.)
    if (tile >= tiles) return;                               // whole block

    // IL: the interleaved k split also for rows that are only 4-byte aligned (K % 4 != 0: the 167 atom features of layer 0):
    // the same 64 contiguous bytes per row and instruction, loaded as unaligned 16-byte pieces; only the piece that
    // straddles the end of the row is loaded element by element.  (The blocked split it replaces ran that projection
    // at 22 us for 0.6 GFLOP.)
    constexpr bool IL = VEC || (KQ % 4 == 0);
    auto load_rows = [&](int64_t t, float (&xa)[KQ]) {
        int64_t row = t * kLinRows + w * 16 + i;
        row = row < M ? row : M - 1;
        const float* src = X + row * K + (IL ? 4 * kq : kq * KQ);
        if (VEC) {
#pragma unroll
            for (int s = 0; s < KQ / 4; ++s) {
                const float4 v = ld4(src + s * 16);
                xa[4 * s + 0] = v.x; xa[4 * s + 1] = v.y; xa[4 * s + 2] = v.z; xa[4 * s + 3] = v.w;
            }
        } else if (IL) {
#pragma unroll
            for (int s = 0; s < KQ / 4; ++s) {
                const int col = 16 * s + 4 * kq;
                if (col + 3 < K) {
                    const f32x4_u4 v = *reinterpret_cast<const f32x4_u4*>(src + s * 16);
                    xa[4 * s + 0] = v.v[0]; xa[4 * s + 1] = v.v[1]; xa[4 * s + 2] = v.v[2]; xa[4 * s + 3] = v.v[3];
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c) xa[4 * s + c] = (col + c < K) ? src[s * 16 + c] : 0.f;
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < KQ; ++s) xa[s] = (kq * KQ + s < K) ? src[s] : 0.f;
        }
    };

    float cur[KQ], nxt[KQ];
    {   // stage Bt [4*KQ][this half's 64 columns] -> LDS with 16-byte loads; the first A rows ride in the same round trip
        constexpr int N4 = 4 * KQ * 16;                 // float4 count
        constexpr int PER = (N4 + kLinThreads - 1) / kLinThreads;
        float4 v[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int idx = tid + q * kLinThreads, k = idx >> 4, n4 = idx & 15;
            v[q] = (idx < N4 && k < K) ? ld4(Bt + (size_t)k * 128 + 64 * wc + n4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        load_rows(tile, cur);
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int idx = tid + q * kLinThreads, k = idx >> 4, n4 = idx & 15;
            if (idx < N4) st4(sBt + k * kLinLd + n4 * 4, v[q]);
        }
    }
    // this lane's four columns of bias and of the two attention vectors stay in registers for every tile
    const int col = 64 * wc + 4 * i;
    const float4 bv = bias ? ld4(bias + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int ns_d = ns.att ? FN_D / ns.heads : FN_D, ns_head = col / ns_d;
    float4 a_dst = make_float4(0.f, 0.f, 0.f, 0.f), a_src = a_dst;
    if (ns.att) {
        a_dst = ld4(ns.att + ns_head * ns.att_w + ns.dst_off + col % ns_d);
        a_src = ld4(ns.att + ns_head * ns.att_w + ns.src_off + col % ns_d);
    }
    const float ik = mk.p < 1.f ? 1.f / (1.f - mk.p) : 0.f;
    float4 ra_a[4];
    if (RA) {
#pragma unroll
        for (int hh = 0; hh < 4; ++hh) ra_a[hh] = ra.z ? ld4(ra.a + hh * ra.lda + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    // MFMA tile t of a wave covers the columns {4 i + t}: one 16-byte LDS read per step feeds all four tiles
    const float* bbase = sBt + (IL ? 4 * kq : kq * KQ) * kLinLd + 4 * i;
    auto brow = [](int s) { return IL ? 16 * (s >> 2) + (s & 3) : s; };       // LDS row of MFMA step s, relative to bbase
    for (;;) {
        const int64_t next = tile + stride;
        const bool more = next < tiles;
        if constexpr (PF) load_rows(more ? next : tile, nxt);
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // B operands are read four steps (16 MFMAs) ahead, in two register groups
        constexpr int NG = (KQ + 3) / 4;
        float4 bg[2][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) bg[0][q] = q < KQ ? *reinterpret_cast<const float4*>(bbase + brow(q) * kLinLd) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int sn = 4 * (g + 1) + q;
                    if (sn < KQ) bg[(g + 1) & 1][q] = *reinterpret_cast<const float4*>(bbase + brow(sn) * kLinLd);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int sc = 4 * g + q;
                if (sc < KQ) {
                    const float4 b = bg[g & 1][q];
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[sc], b.x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[sc], b.y, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[sc], b.z, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[sc], b.w, acc[3], 0, 0, 0);
                }
            }
        }
        // acc[t][r] is (row kq*4 + r, column 4 i + t) of the wave's 16 x 64 tile
        __builtin_amdgcn_sched_barrier(0);
        const int64_t r0 = tile * kLinRows + w * 16 + kq * 4;
        // the output rows are a next-launch table (store policy: fn_internal.h): the row tile's first row is the wave-uniform base, so the
        // 32-bit byte offset stays inside the tile whatever M is
        float* const Yt = Y + tile * (kLinRows * 128);
        const uint32_t yoff = (uint32_t)((w * 16 + kq * 4) * 128 + col) * 4u;
        float pd[4], ps[4];
        if constexpr (CU) {
            // one-pass backward: the gate's saved output, the raw / second output rows and the edge-term gradient of all four rows
            // in ONE round trip (row by row, as below, each row's loads wait behind the previous row's stores)
            static_assert(!CU || RA, "the row-dots epilogue rides in the RowAdd instances");
            const bool gate = mk.y && mk.relu;           // (the engine's gates are all relu(dropout(.)): no Philox replay here.  Round 4: for the
                                                         // bond level, whose raw rows are loaded for the dots anyway, the gate regenerated from
                                                         // out > 0 and a Philox call per lane and row instead of reading y -- 13.6 MB of 124 less
                                                         // per inner layer -- measured slower, 32.9 -> 37.5 us: 168 VGPRs with spills; not kept)
            const float sc = mk.p > 0.f ? ik : 1.f;
            const int cu_hd = cu.c ? col / (FN_D / cu.heads) : 0;
            float sgv[4];
            // all four rows' operands in one round trip (64 registers: the kernel runs three waves per SIMD)
            constexpr int CR = kCuRows;
#pragma unroll
            for (int hb = 0; hb < 4; hb += CR) {
                float4 yv[CR], ov[CR], o2v[CR], zv[CR];
#pragma unroll
                for (int q = 0; q < CR; ++q) {
                    const int r = hb + q;
                    const int64_t row = r0 + r < M ? r0 + r : M - 1;
                    const int64_t at = row * 128 + col;
                    yv[q] = gate ? ld4(mk.y + at) : make_float4(1.f, 1.f, 1.f, 1.f);
                    ov[q] = cu.c && cu.out ? ld4(cu.out + at) : make_float4(0.f, 0.f, 0.f, 0.f);
                    o2v[q] = cu.c && cu.out2 ? ld4(cu.out2 + at) : make_float4(0.f, 0.f, 0.f, 0.f);
                    zv[q] = ra.z ? ld4(ra.z + row * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                    sgv[r] = cu.c && cu.out2 ? cu.sigma[row * cu.heads + cu_hd] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < CR; ++q) {
                    const int r = hb + q;
                    float4 o = make_float4(acc[0][r] + bv.x, acc[1][r] + bv.y, acc[2][r] + bv.z, acc[3][r] + bv.w);
                    if (gate) {
                        o.x = yv[q].x > 0.f ? o.x * sc : 0.f; o.y = yv[q].y > 0.f ? o.y * sc : 0.f;
                        o.z = yv[q].z > 0.f ? o.z * sc : 0.f; o.w = yv[q].w > 0.f ? o.w * sc : 0.f;
                    }
                    fma4(o, zv[q].x, ra_a[0]);  fma4(o, zv[q].y, ra_a[1]);  fma4(o, zv[q].z, ra_a[2]);  fma4(o, zv[q].w, ra_a[3]);
                    if (r0 + r < M) st4_next(Yt, yoff + r * 512, o);
                    pd[r] = dot4(o, cu.out ? ov[q] : yv[q]);
                    ps[r] = dot4(o, o2v[q]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (cu.c) {          // per-head sums over the head's cu_d / 4 neighbouring lanes of the 16-lane DPP row, as for the node scalars
                const int cu_d = FN_D / cu.heads;
                const float cu_scale = cu.out ? 1.f : (mk.p > 0.f && mk.p < 1.f ? 1.f - mk.p : 1.f);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (cu_d >= 64) pd[r] += dpp_mov<kDppMirror>(pd[r]);
                    if (cu_d >= 32) pd[r] += dpp_mov<kDppHalfMirror>(pd[r]);
                    pd[r] += dpp_mov<kDppXor2>(pd[r]);
                    pd[r] += dpp_mov<kDppXor1>(pd[r]);
                    if (cu_d >= 64) ps[r] += dpp_mov<kDppMirror>(ps[r]);
                    if (cu_d >= 32) ps[r] += dpp_mov<kDppHalfMirror>(ps[r]);
                    ps[r] += dpp_mov<kDppXor2>(ps[r]);
                    ps[r] += dpp_mov<kDppXor1>(ps[r]);
                    if ((4 * i) % cu_d == 0 && r0 + r < M) {
                        const float cc = cu_scale * pd[r];
                        cu.c[(r0 + r) * cu.heads + cu_hd] = cc;
                        cu.u[(r0 + r) * cu.heads + cu_hd] = ps[r] - cc * sgv[r];
                    }
                }
            }
        } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float4 o = make_float4(acc[0][r] + bv.x, acc[1][r] + bv.y, acc[2][r] + bv.z, acc[3][r] + bv.w);
            pd[r] = dot4(o, a_dst);
            ps[r] = dot4(o, a_src);
            if (r0 + r < M) {
                float4 yy = make_float4(0.f, 0.f, 0.f, 0.f);
                if (mk.y) {      // backward of act(dropout(.)) fused into the input-gradient GEMM: o *= mask * (y > 0)
                    const int64_t e4 = (r0 + r) * 32 + 16 * wc + i;              // Philox block = element / 4
                    if (mk.relu) {
                        // y = relu(dropout(x)) is positive only where the element was kept AND passed the ReLU: the saved
                        // output already encodes the mask, so the Philox stream is not replayed (240 VALU ops a tile)
                        yy = ld4(mk.y + e4 * 4);
                        const float sc = mk.p > 0.f ? ik : 1.f;
                        o.x = yy.x > 0.f ? o.x * sc : 0.f; o.y = yy.y > 0.f ? o.y * sc : 0.f;
                        o.z = yy.z > 0.f ? o.z * sc : 0.f; o.w = yy.w > 0.f ? o.w * sc : 0.f;
                    } else if (mk.p > 0.f) {
                        const uint4 rnd = philox4x32(mk_base + (uint64_t)e4, mk.seed);
                        o.x *= keep_scale(rnd.x, mk.p, ik); o.y *= keep_scale(rnd.y, mk.p, ik);
                        o.z *= keep_scale(rnd.z, mk.p, ik); o.w *= keep_scale(rnd.w, mk.p, ik);
                    }
                }
                if (RA) {
                    if (ra.z) {          // after the gate: the term is a gradient w.r.t. the pre-activation row itself
                        const float4 z = ld4(ra.z + (r0 + r) * 4);
                        fma4(o, z.x, ra_a[0]);  fma4(o, z.y, ra_a[1]);  fma4(o, z.z, ra_a[2]);  fma4(o, z.w, ra_a[3]);
                    }
                }
                if (POL) st4_next(Yt, yoff + r * 512, o); else st4(Y + (r0 + r) * 128 + col, o);
            }
            __builtin_amdgcn_sched_barrier(0);               // one row at a time: four interleaved Philox chains cost 60 VGPRs
        }
        }
        if (!CU && ns.att) {     // node scalars: a head's ns_d columns are ns_d/4 neighbouring lanes of the 16-lane DPP row
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (ns_d >= 64) { pd[r] += dpp_mov<kDppMirror>(pd[r]); ps[r] += dpp_mov<kDppMirror>(ps[r]); }
                if (ns_d >= 32) { pd[r] += dpp_mov<kDppHalfMirror>(pd[r]); ps[r] += dpp_mov<kDppHalfMirror>(ps[r]); }
                pd[r] += dpp_mov<kDppXor2>(pd[r]); ps[r] += dpp_mov<kDppXor2>(ps[r]);
                pd[r] += dpp_mov<kDppXor1>(pd[r]); ps[r] += dpp_mov<kDppXor1>(ps[r]);
                if ((4 * i) % ns_d == 0 && r0 + r < M) {
                    ns.s_dst[(r0 + r) * ns.heads + ns_head] = pd[r];
                    ns.s_src[(r0 + r) * ns.heads + ns_head] = ps[r];
                }
            }
        }
        if (!more) break;
        if constexpr (PF) {
#pragma unroll
            for (int s = 0; s < KQ; ++s) cur[s] = nxt[s];
        } else {
            load_rows(next, cur);
        }
        tile = next;
    }
}


using fni::LinTask;
using fni::LinTasks;
// ---- an attention pass and the projection GEMMs that do not depend on it, in ONE launch.
// Inside a layer the chain is  projections -> bond + fragment-bond levels -> atom level, but only a third of it is a true
// dependency: the atom projection of layer l needs layer l-1's atom level and nothing of layer l's bond levels, and the bond /
// fragment-bond projections of layer l+1 need layer l's bond levels and nothing of its atom level (the backward mirrors this:
// the atom input-gradient product does not wait for the bond levels' passes, and theirs not for the next layer's atom pass).
// The attention passes are bound by dependent round trips with the matrix cores idle, the projections are a few microseconds
// of MFMA work behind a launch floor of their own -- so the GEMM tiles ride along as extra workgroups of the attention launch
// (one 64 x 64 tile each, the k_linear128_multi body) and the layer loses a kernel boundary per pass.
template <bool CU = false>
__device__ __forceinline__ void lin_side_block(float* sBt, const LinTasks& T, int b) {
    int ti = 0;
    while (ti + 1 < T.n && b >= T.t[ti + 1].first) ++ti;
    const LinTask& t = T.t[ti];
    linear128_body<32, true, false, true, CU>(sBt, t.X, 128, t.Bt, t.bias, t.Y, t.M, t.mk, t.ns, b - t.first, t.nblk, t.ra, t.cu, t.n_real);
}
// Which workgroup is which: the GEMM workgroups are blocks [T.base, T.base + T.total) of the launch -- first, so that the
// dispatcher starts them before the attention workgroups (measured best of first / last / interleaved: profiles/r02e_colaunch_ab.txt).
// Returns the role's own block index in *idx.
__device__ __forceinline__ bool lin_side_role(const LinTasks& T, int gat_base, int* idx) {
    const int b = (int)blockIdx.x - T.base;
    if ((unsigned)b < (unsigned)T.total) { *idx = b;  return true; }
    *idx = (int)blockIdx.x - gat_base;
    return false;
}

// dynamic LDS of a launch that carries side blocks: the [128][64] operand tile of one column half
constexpr size_t kLinSideLds = (size_t)(4 * 32 * kLinLd) * sizeof(float);
static_assert(kLinSideLds <= 64 * 1024, "the co-launched GEMM tile fits the default dynamic LDS limit");
