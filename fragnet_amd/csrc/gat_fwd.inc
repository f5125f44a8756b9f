// gat_fwd.inc -- device code of the attention forward (included, inside the anonymous namespace, by gat_fwd.hip, gat_fwd_lin.hip, by
// encoder.hip -- for the molecule-resident fragment tail, which runs the row core on its own rows -- and by fragnet_hip.hip, for
// k_node_scalars and the helpers gat_bwd_two.inc shares).  Templates only.  GatFwdArgs: fn_internal.h.
// folded edge-embedding weights: Wf[h][k] = sum_c att[h, mid+c] * embW[c,k],  Wf[h][K] = sum_c att[h, mid+c] * embb[c]
__device__ __forceinline__ void fold_edge_embed(const fn_edge_term& et, const float* att, int att_w, int H,
                                                float (*sWf)[kWfLd]) {
    // one wave per output scalar, lanes over the d_e-long dot product (two loads per lane, no serial chain: every
    // block of the launch pays this prologue before its first node)
    if (et.mode == 2) {
        const int ne = H * (et.K + 1);
        const int wid = threadIdx.x >> 6, l64 = threadIdx.x & 63, nw = blockDim.x >> 6;
        for (int i = wid; i < ne; i += nw) {
            const int hh = i / (et.K + 1), k = i % (et.K + 1);
            float part = 0.f;
            for (int c = l64; c < et.d_e; c += 64)
                part = fmaf(att[hh * att_w + et.mid_off + c], (k < et.K) ? et.embW[c * et.K + k] : et.embb[c], part);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
            if (l64 == 0) sWf[hh][k] = part;
        }
    }
    __syncthreads();
}

// edge term of the logit for the edge at destination-sorted position pos.  Per-edge arrays are HEAD-MAJOR
// ([H][m], [K][m]) so that the two consecutive edges a lane owns are one 8-byte load.
template <int H>
__device__ __forceinline__ float edge_term_at(int pos, int head, int64_t m, const fn_edge_term& et, const float (*sWf)[kWfLd]) {
    if (et.mode == 0) return et.s_sorted[(size_t)head * m + pos];
    float e = sWf[head][et.K];
    for (int k = 0; k < et.K; ++k) e = fmaf(et.x_sorted[(size_t)k * m + pos], sWf[head][k], e);
    return e;
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_node_scalars(const float* __restrict__ h, const float* __restrict__ att,
                                                         int att_w, int dst_off, int src_off,
                                                         float* __restrict__ s_dst, float* __restrict__ s_src, int64_t n) {
    constexpr int LPH = 32 / H;
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH;
    const float4 ad = ld4(att + head * att_w + dst_off + j * 4);
    const float4 as = ld4(att + head * att_w + src_off + j * 4);
    int64_t g0, g1;
    block_groups(n, kRows, g0, g1);
    for (int64_t gi = g0; gi < g1; ++gi) {
        const int64_t r = gi * kRows + (threadIdx.x >> 5);
        if (r >= n) continue;
        const float4 x = ld4(h + r * FN_D + lane * 4);
        const float pd = head_sum<LPH>(dot4(x, ad));
        const float ps = head_sum<LPH>(dot4(x, as));
        if (j == 0) { s_dst[r * H + head] = pd; s_src[r * H + head] = ps; }
    }
}

// What bounds these kernels at molecule-batch sizes is neither HBM nor L2 bandwidth but the CHAIN of dependent
// global round trips a row needs (row extent -> edge ids/terms -> source rows + source scalars -> store), ~1.2 us
// each when ~100 rows per CU is all the work there is (ablation in DESIGN.md: gathering the same rows from an LDS
// window instead of L2 changed nothing; an empty skeleton with two round trips already costs 9.5 us).  So:
//  * every per-edge scalar is fetched ONCE by the lane that owns the edge -- lane j of a head group owns the
//    consecutive in-edges 2j and 2j+1, one 8-byte load per array -- and handed round through LDS-crossbar
//    broadcasts (__shfl), never through repeated uniform global loads (TA: one wave instruction per ~16 cycles);
//  * up to eight source rows are in flight per half-wave before the softmax needs anything;
//  * a half-wave owns R CONSECUTIVE rows and software-pipelines them: while row i's gathers fly, the edge data of
//    row i+1 and the extent of row i+2 are already being fetched, so a row costs one round trip, not four.
struct FwdExtent { int beg, deg; float sd; int mk; };         // deg < 0: no row; mk: the row's mask byte (kind 4 only, else 0)
struct FwdEdges { int src0, src1; float z0, z1; };            // the lane's two in-edges: source ids, edge terms
struct FwdRaw {                                               // the same, as loaded (folded one iteration later)
    int pos;
    i32x2u sp;
    f32x2u e[FN_MAX_EDGE_K];
};
template <int NE> struct FwdRawT {                            // sized to the loads a kernel instance makes
    int pos;
    i32x2u sp;
    f32x2u e[NE];
};
// The hot loop is STRAIGHT-LINE: every load is unconditional (addresses clamped into the arrays, results masked
// afterwards).  A load inside a divergent branch whose value is used inside that branch makes the compiler wait
// for vmcnt(0) right there -- which serialised the row gathers, the two source-scalar gathers and the prefetches
// into separate round trips in the previous version of this kernel.
// KL: 0 = the edge term is a stored per-edge scalar (mode 0); 1 / FN_MAX_EDGE_K = folded Linear(K -> d) of a raw
// attribute with K == 1 / K <= FN_MAX_EDGE_K (attribute columns beyond K are re-loads of column K-1 with weight 0,
// so that the number of loads is a compile-time constant and none of them sits in a branch).
using fni::GatFwdArgs;
// rows [blk0, te) of the level, taken interleaved by the block's half-waves (row = blk0 + i * kRows + hw, i < rows_per_hw);
// sWf: the folded edge-embedding weights (KL != 0), already in LDS
// O2 is the forward's KIND: 0 plain; 1 with the second output (out2, sigma) for the one-pass backward; 2 the same for the ENGINE's
// training launches, whose run-time constants are then compile-time ones -- probabilities edge-major, no probs_orig, a level of at
// least two edges, and an epilogue (if any) that is relu(dropout(.)) with p > 0 (fwd_kind_tr() on the host checks exactly that);
// 3 the plain forward of the engine's EVALUATION launches: probabilities head-major, no probs_orig, >= 2 edges, an epilogue (if any)
// that is a ReLU without dropout (fwd_kind_ev());
// 4 the MASKED evaluation forward (fn_encoder_forward_masked): kind 3's constants -- except that a level may have fewer than two edges,
// a batch of replicas of one small molecule has such levels -- plus one byte per destination row (rmask, 1 = this row is zero for
// every reader).  The byte travels with the row's extent, two rows ahead, and acts on the finished row in registers, before the raw
// store, the row-dots epilogue and the activation epilogue: none of the three sees memory in between.
// Round 6: a third of this loop's issue slots were scalar bookkeeping and branches (profiles/r06_isa_mix.md); the tests of these
// uniform flags inside the row loop were part of it: 0.761 -> 0.750 ms per step with them folded, bit-identical results.
template <int H, int KL, bool RD = false, int O2 = 0>
__device__ __forceinline__ void gat_fwd_rows(const GatFwdArgs& A, float (*sWf)[kWfLd], int blk0, int te, int rows_per_hw,
                                             const uint8_t* __restrict__ rmask = nullptr) {
    const float* __restrict__ h = A.h;
    const float* __restrict__ s_dst = A.s_dst;
    const float* __restrict__ s_src = A.s_src;
    const fn_edge_term& et = A.et;
    const fn_gat_plan& pl = A.pl;
    const float slope = A.slope;
    float* __restrict__ out = A.out;
    float* __restrict__ p_sorted = A.p_sorted;
    constexpr bool MK = O2 == 4;
    constexpr bool TR = O2 == 2, EV = O2 == 3 || MK, KC = TR || EV;      // KC: a kind whose uniform flags are constants
    float* __restrict__ probs_orig = KC ? nullptr : A.probs_orig;
    const bool wp = TR || p_sorted != nullptr;            // the engine's evaluation launches of a pass nobody differentiates save no probabilities
    const fn_act_epilogue& ep = A.ep;
    float* __restrict__ out2 = A.out2;
    constexpr bool o2 = O2 == 1 || O2 == 2;   // the second output (out2, sigma) is a compile-time variant: its accumulators cost registers
    constexpr int LPH = 32 / H;
    constexpr int NE = KL ? KL : 1;                       // 8-byte edge loads per lane and row
    // source rows gathered in one round trip.  12 (the bond graph's top degree class, as the one-pass backward has it) measured SLOWER
    // here: the forward kernels sit at the 128-register mark of four waves per SIMD and the four extra rows spill (plain 15.4 -> 15.8 us,
    // with the second output 17.4 -> 20.5 us at B = 512)
    constexpr int NG = 8;
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH;
    const int m = (int)pl.m, n = (int)pl.n;
    const int K = KL ? et.K : 0;
    float wf[NE];                                         // this head's folded edge-embedding weights
#pragma unroll
    for (int k = 0; k < NE; ++k) wf[k] = (KL && k < K) ? sWf[head][k] : 0.f;
    const float wbias = KL ? sWf[head][K] : 0.f;
    const int tb = blk0 + (int)(threadIdx.x >> 5);
    const bool pairs = (KC && !MK) ? true : m >= 2;       // paired edge loads need two edges in the level
    const float* e_sorted = KL ? nullptr : et.s_sorted + (size_t)head * m;
    const int nr = A.n_real ? *A.n_real : n;              // rows behind it: padding of a static-shape batch -> rows without edges
    // kind 4: a level without a mask of its own (only the atoms are masked, say) reads the bytes of its row extents instead and
    // discards them -- the load stays unconditional, no branch in the row loop
    const uint8_t* __restrict__ mk_p = (MK && rmask) ? rmask : reinterpret_cast<const uint8_t*>(pl.rowptr_d);
    const int mk_on = (MK && rmask) ? 1 : 0;

    auto load_extent = [&](int t) {
        const int tc = t < n ? t : n - 1;
        const i32x2u rp = ldp(pl.rowptr_d + tc);
        FwdExtent x;
        x.beg = rp.x - pl.pos_base_d;
        x.deg = t < te ? (t < nr ? rp.y - rp.x : 0) : -1;
        x.sd = s_dst[(uint32_t)tc * H + head];
        x.mk = 0;
        if constexpr (MK) x.mk = mk_p[(uint32_t)tc] ? mk_on : 0;
        return x;
    };
    auto issue_edges = [&](const FwdExtent& x, FwdRawT<NE>& r) {
        int pos = x.beg + 2 * j;
        pos = pos > m - 2 ? m - 2 : pos;
        pos = pos < 0 ? 0 : pos;
        r.pos = pos;
        if (!pairs) { r.sp.x = r.sp.y = 0;  return; }
        r.sp = ldp(pl.src_d + pos);
        if (KL == 0) r.e[0] = ldp(e_sorted + pos);
        else {
#pragma unroll
            for (int k = 0; k < NE; ++k) r.e[k] = ldp(et.x_sorted + (size_t)(k < K ? k : K - 1) * m + pos);
        }
    };
    auto fold_edges = [&](const FwdExtent& x, const FwdRawT<NE>& r) {
        FwdEdges e;
        float za, zb;
        if (KL == 0) { za = r.e[0].x;  zb = r.e[0].y; }
        else {
            za = zb = wbias;
#pragma unroll
            for (int k = 0; k < NE; ++k) { za = fmaf(r.e[k].x, wf[k], za);  zb = fmaf(r.e[k].y, wf[k], zb); }
        }
        const bool shifted = x.beg + 2 * j != r.pos;      // only the very last edge of the level: its pair starts one early
        e.src0 = shifted ? r.sp.y : r.sp.x;  e.z0 = shifted ? zb : za;
        e.src1 = r.sp.y;  e.z1 = zb;
        return e;
    };

    const uint64_t rng_base = ep.offset + ((ep.y && ep.p > 0.f && ep.offset_dev) ? *ep.offset_dev : 0);
    FwdRawT<NE> raw;
    FwdExtent cur = load_extent(tb);
    issue_edges(cur, raw);
    FwdExtent nxt = load_extent(tb + kRows);
    FwdEdges ed = fold_edges(cur, raw);
    // drain the prologue's loads here: otherwise the compiler, unable to tell the first iteration from the others,
    // puts a vmcnt(0) at the loop head, where it also waits for the previous iteration's STORES
    asm volatile("" ::"v"(nxt.sd), "v"(nxt.beg), "v"(nxt.deg), "v"(ed.src0), "v"(ed.src1), "v"(ed.z0), "v"(ed.z1));
    for (int t = tb; t < tb + kRows * rows_per_hw; t += kRows) {     // uniform trip count: both half-waves of a wave stay in step
        const int beg = cur.beg, deg = cur.deg;
        const bool fast = pairs && deg >= 0 && deg <= 2 * LPH;
        const bool has0 = fast && 2 * j < deg, has1 = fast && 2 * j + 1 < deg;
        // a lane without an edge gathers the destination row itself (weight 0): always a row this launch may read -- the
        // molecule-resident callers (mol_tail.inc) have only their own molecule's rows written, and 0 * stale NaN is NaN
        const int src0 = has0 ? ed.src0 : (t < n ? t : n - 1), src1 = has1 ? ed.src1 : src0;
        // one round trip: next row's edge data, the row after's extent, this row's source rows and source scalars
        issue_edges(nxt, raw);
        const FwdExtent nn = load_extent(t + 2 * kRows);
        const int rd_p = RD ? A.rd_pos[t < n ? t : n - 1] : 0;            // requested with the gathers, consumed after them
        // source rows in flight per half-wave: 4, 8 or NG (wave-uniform tiers; NG = 12 for the single-attribute class = the bond graph,
        // whose rows between two four-valent atoms have 10 or 12 in-edges: 28 % of the ESOL-shape rows); rows beyond the tier take a
        // second, dependent round trip further down
        const bool wide = __any(fast && deg > 4), wide2 = NG > 8 && __any(fast && deg > 8);
        const bool live = __any(!fast || deg > 0);        // false: neither row of the wave has an edge (padding, isolated nodes) -> nothing to gather
        float4 r0[NG];
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
                r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
            }
        }
        // (a tier at 6 -- 57 % of the bond graph's rows have six in-edges: two loads less for the waves whose two rows stop there)
        const bool wide8 = __any(fast && deg > (A.tier6 ? 6 : 4));
        if (wide) {
#pragma unroll
            for (int i = 4; i < 6; ++i) {
                const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
                r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
            }
        }
        if (wide8) {
#pragma unroll
            for (int i = 6; i < 8; ++i) {
                const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
                r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
            }
        }
        if (wide2) {
#pragma unroll
            for (int i = 8; i < NG; ++i) {
                const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
                r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
            }
        }
        const float ss0 = ld1_off(s_src, ((uint32_t)src0 * H + head) * 4);
        const float ss1 = ld1_off(s_src, ((uint32_t)src1 * H + head) * 4);

        const float z0 = ed.z0 + cur.sd + ss0, z1 = ed.z1 + cur.sd + ss1;
        const float l0 = has0 ? fmaxf(z0, slope * z0) : -INFINITY;       // LeakyReLU, 0 < slope < 1
        const float l1 = has1 ? fmaxf(z1, slope * z1) : -INFINITY;
        const float mx = head_max<LPH>(fmaxf(l0, l1));
        const float e0 = has0 ? __expf(l0 - mx) : 0.f;
        const float e1 = has1 ? __expf(l1 - mx) : 0.f;
        const float inv = __builtin_amdgcn_rcpf(head_sum<LPH>(e0 + e1));
        const float p0 = has0 ? e0 * inv : 0.f;
        const float p1 = has1 ? e1 * inv : 0.f;
        // everything issued above has arrived by now (loads return in order): fold the next row's edge data BEFORE
        // this row's stores, so that nothing at the top of the next iteration has to wait behind those stores
        const FwdEdges ed_n = fold_edges(nxt, raw);
        const float sd_cur = cur.sd;
        const int mk_cur = cur.mk;
        cur = nxt;  nxt = nn;  ed = ed_n;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), acc2 = acc;
        // signed probabilities (sign bit = the LeakyReLU branch z <= 0): what the backward reads, and what out2 weighs by
        const float sp0 = has0 ? (z0 > 0.f ? p0 : -p0) : 0.f, sp1 = has1 ? (z1 > 0.f ? p1 : -p1) : 0.f;
        auto lam = [&](float sp) { return sp < 0.f ? -slope * sp : sp; };        // lambda_e p_e
        if (!live) {
            // (no row of this wave has an edge: r0 was not loaded)
        } else if constexpr (!o2) {
#pragma unroll
            for (int i = 0; i < 4; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            if (wide) {
#pragma unroll
                for (int i = 4; i < 6; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
            if (wide8) {
#pragma unroll
                for (int i = 6; i < 8; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
            if (wide2) {
#pragma unroll
                for (int i = 8; i < NG; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float spk = __shfl((i & 1) ? sp1 : sp0, i >> 1, LPH);
                fma4(acc, fabsf(spk), r0[i]);
                fma4(acc2, lam(spk), r0[i]);
            }
            if (wide) {
#pragma unroll
                for (int i = 4; i < 6; ++i) {
                    const float spk = __shfl((i & 1) ? sp1 : sp0, i >> 1, LPH);
                    fma4(acc, fabsf(spk), r0[i]);
                    fma4(acc2, lam(spk), r0[i]);
                }
            }
            if (wide8) {
#pragma unroll
                for (int i = 6; i < 8; ++i) {
                    const float spk = __shfl((i & 1) ? sp1 : sp0, i >> 1, LPH);
                    fma4(acc, fabsf(spk), r0[i]);
                    fma4(acc2, lam(spk), r0[i]);
                }
            }
            if (wide2) {
#pragma unroll
                for (int i = 8; i < NG; ++i) {
                    const float spk = __shfl((i & 1) ? sp1 : sp0, i >> 1, LPH);
                    fma4(acc, fabsf(spk), r0[i]);
                    fma4(acc2, lam(spk), r0[i]);
                }
            }
        }
        float sg = 0.f;
        if constexpr (o2) sg = head_sum<LPH>(lam(sp0) + lam(sp1));
        if (fast) {
            const int pos0 = beg + 2 * j;
            if (TR || (!EV && A.p_edge_major)) {
                if (has0 && wp) st1_late(p_sorted, ((uint32_t)pos0 * H + head) * 4u, sp0);        // (store policy: fn_internal.h)
                if (has1 && wp) st1_late(p_sorted, ((uint32_t)(pos0 + 1) * H + head) * 4u, sp1);
            } else if (wp) {
                float* pdst = p_sorted + (size_t)head * m + pos0;
                if (has1) stp(pdst, sp0, sp1);
                else if (has0) pdst[0] = sp0;
            }
            if (probs_orig) {
                if (has0) probs_orig[(size_t)pl.eid_d[pos0] * H + head] = p0;
                if (has1) probs_orig[(size_t)pl.eid_d[pos0 + 1] * H + head] = p1;
            }
            for (int k0 = NG; k0 < deg; k0 += 4) {        // in-degree NG + 1 .. 2*LPH
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + i;
                    const int sk = __shfl((i & 1) ? src1 : src0, k >> 1, LPH);
                    const float spk = __shfl((i & 1) ? sp1 : sp0, k >> 1, LPH);
                    const float4 row = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
                    fma4(acc, fabsf(spk), row);
                    if constexpr (o2) fma4(acc2, lam(spk), row);
                }
            }
        } else if (deg >= 0) {
            // rare high in-degree node (or a level with a single edge): every lane walks the edge list (three passes)
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            sg = 0.f;
            auto logit = [&](int pos, int& sk) {
                sk = pl.src_d[pos];
                const float z = sd_cur + s_src[(size_t)sk * H + head] + edge_term_at<H>(pos, head, m, et, sWf);
                return z > 0.f ? z : slope * z;
            };
            int sk = 0;
            float mxs = -INFINITY;
            for (int i = 0; i < deg; ++i) mxs = fmaxf(mxs, logit(beg + i, sk));
            float den = 0.f;
            for (int i = 0; i < deg; ++i) den += expf(logit(beg + i, sk) - mxs);
            for (int i = 0; i < deg; ++i) {
                const float l = logit(beg + i, sk);
                const float p = expf(l - mxs) / den;
                if (j == 0) {
                    if (wp) p_sorted[(TR || (!EV && A.p_edge_major)) ? (size_t)(beg + i) * H + head : (size_t)head * m + beg + i] = l > 0.f ? p : -p;
                    if (probs_orig) probs_orig[(size_t)pl.eid_d[beg + i] * H + head] = p;
                }
                const float4 row = ld4(h + (size_t)sk * FN_D + lane * 4);
                fma4(acc, p, row);
                if constexpr (o2) { const float q = l > 0.f ? p : slope * p;  fma4(acc2, q, row);  sg += q; }
            }
        }
        if constexpr (MK) {      // a masked row is zero for all three readers below (selects, not a product: 0 * inf would be NaN)
            acc.x = mk_cur ? 0.f : acc.x;  acc.y = mk_cur ? 0.f : acc.y;  acc.z = mk_cur ? 0.f : acc.z;  acc.w = mk_cur ? 0.f : acc.w;
        }
        if (deg >= 0) {
            const uint32_t row_off = (uint32_t)t * (FN_D * 4) + lane * 16;          // (n <= 2^23 rows: fits)
            if (out) st4_next(out, row_off, acc);               // raw rows: the next launch reads them; out2 / sigma: only the backward
            if constexpr (o2) {
                st4_late(out2, row_off, acc2);
                if (j == 0) st1_late(A.sigma, ((uint32_t)t * H + head) * 4u, sg);
            }
            if (RD) {            // the next level's edge term from the row in registers (saves a launch that re-reads every row)
                float mine = 0.f;
                const int rdJ = KC ? H : A.rd_J;                 // (the engine's edge term has one row of A per head: a fixed trip count unrolls)
#pragma unroll
                for (int q = 0; q < rdJ; ++q) {
                    // (staging these J rows in LDS once per block instead of loading them per row changed nothing: 31.2 -> 32.1 us)
                    const float dsum = head_sum<32>(dot4(acc, ld4_off(A.rd_A, (uint32_t)(q * A.rd_lda + lane * 4) * 4u)));
                    if (lane == q) mine = dsum;
                }
                if (lane < rdJ) st1_next(A.rd_out, ((uint32_t)lane * (uint32_t)A.rd_m + (uint32_t)rd_p) * 4u, mine);
            }
            if (ep.y) {          // fused act(dropout(.)): same Philox block index (element / 4) as k_dropout_act
                float4 r = acc;
                if (TR || (!EV && ep.p > 0.f)) {
                    const uint4 rnd = philox4x32(rng_base + (uint64_t)t * 32 + lane, ep.seed);
                    const float ik = ep.p < 1.f ? 1.f / (1.f - ep.p) : 0.f;
                    r.x *= keep_scale(rnd.x, ep.p, ik); r.y *= keep_scale(rnd.y, ep.p, ik);
                    r.z *= keep_scale(rnd.z, ep.p, ik); r.w *= keep_scale(rnd.w, ep.p, ik);
                }
                if (KC || ep.relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
                st4_next(ep.y, row_off, r);
            }
        }
    }
}

// a block owns kRows * R consecutive rows; its half-waves take them INTERLEAVED (row = base + i * kRows + hw), so
// that at any moment the block works on kRows neighbouring rows whose source rows overlap (L1 reuse across waves)
template <int H, int KL, bool RD = false, int O2 = 0>
__device__ __forceinline__ void gat_fwd_body(const GatFwdArgs& A, float (*sWf)[kWfLd], int bid, int nblk, const uint8_t* rmask = nullptr) {
    const int n = (int)A.pl.n, per = kRows * A.rows_per_hw;
    const int nr = A.n_real ? *A.n_real : n;
    const int blk0 = xcd_block_real(bid, nblk, A.n_real ? (nr + per - 1) / per : nblk) * per;      // real rows dealt evenly over the XCDs
    if (FN_PAD_BLOCK_EXIT && blk0 >= nr) {
        // a workgroup whose rows are all padding: what the row loop would write for rows without edges -- zero rows (raw, second output,
        // activated), zero sigma, zero edge-term dots -- without the loop (softmax bookkeeping, Philox, the dots: ~70 % of a real row)
        const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5, end = blk0 + per < n ? blk0 + per : n;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int t = blk0 + hw; t < end; t += kRows) {
            if (A.out) st4(A.out + (size_t)t * FN_D + lane * 4, zero);
            if constexpr (O2 == 1 || O2 == 2) {
                st4(A.out2 + (size_t)t * FN_D + lane * 4, zero);
                if (lane < H) A.sigma[(size_t)t * H + lane] = 0.f;
            }
            if (RD) { if (lane < A.rd_J) A.rd_out[(size_t)lane * A.rd_m + A.rd_pos[t]] = 0.f; }
            if (A.ep.y) st4(A.ep.y + (size_t)t * FN_D + lane * 4, zero);
        }
        return;
    }
    fold_edge_embed(A.et, A.att, A.att_w, H, sWf);
    gat_fwd_rows<H, KL, RD, O2>(A, sWf, blk0, blk0 + per < n ? blk0 + per : n, A.rows_per_hw, rmask);
}

