// gat_bwd_one.inc -- the backward of an attention level as ONE source-owner pass (round 4; included by gat_bwd_one.hip, its own
// translation unit since round 5; the argument structs live in fn_internal.h).
//
// Autograd of gat2.py:146-169 (and 196-219, 250-268, 286-312), SURVEY Appendix C, per head:
//     dp_e = <g[t], h[s]>,  dz_e = lambda_e p_e (dp_e - c_t),  c_t = sum_{e'->t} p_e' dp_e',  lambda_e = 1 (z_e > 0) or the slope
//     g_h[s] = sum_{e: src = s} p_e g[t_e] + g_s_dst[s] a_dst + (sum_{e: src = s} dz_e) a_src,   g_s_dst[t] = sum_{e -> t} dz_e
// The two-pass kernels (k_gat_bwd_dst / k_gat_bwd_src) gather every h[src] row only to form dp_e and c_t, hand (p, dz) to the
// source order through memory and gather every g[dst] row again.  Two node-local identities remove the destination pass:
//     out[t]  = sum_e p_e h[s_e]            =>  c_t        = <g[t], out[t]>                      (the forward's raw output row)
//     out2[t] = sum_e lambda_e p_e h[s_e]   =>  g_s_dst[t] = <g[t], out2[t]> - c_t sigma_t,  sigma_t = sum_e lambda_e p_e
// out2 / sigma are a second output of the forward kernel (one more row store per node), c and g_s_dst are per-head dots of rows
// the producer of g has at hand (the input-gradient GEMM's epilogue, or k_gat_cu below).  What remains is ONE pass in which the
// half-wave that owns source row s keeps h[s] in registers, gathers g[t] of its out-edges (as the source pass always did) and the
// per-edge scalars p (by destination-order position) and c (by destination node), and produces every output of the level:
// g_h, the edge-term gradient (original / destination order, or the lane's share of sum dz (x, 1)), and both attention-vector
// partials.  One 102-MB gather sweep, the scattered (p, dz) stores and the pz_src exchange of the two-pass backward are gone.

using fni::GatBwdOneArgs;

template <int NX> struct OneRaw {
    int pos;
    i32x2u tp, dq;          // destination nodes, positions in the destination order
    f32x2u x[NX ? NX : 1];  // raw edge attributes in source order (mode 2 with x_src; unused otherwise)
};

// source rows [blk0, se) interleaved over the block's RB half-waves; bid: the block's slot (row) in part_a / part_e
//
// DF ("deferred", round 5): an OPERATOR-level form (fn_gat_bwd_one_f32 with dz_em, four heads) that the engine does not use -- its
// own deferred backward was retired (FN_TUNE_RETIRED_29); the single-level kernel keeps the flag because the benchmark times the
// operator with it.  The kernel does not read g_s_dst at all -- so the forward needs no second output (out2 / sigma) and nobody
// computes <g, out2>.  It leaves the two terms that need it OUT of its results and writes dz at the edges' destination-order slots
// instead (dz_em [m][H]: one 16-byte line per edge, a node's in-edges contiguous).  The caller completes them: k_gsd_seg
// (fn_gat_gsd_f32) forms g_s_dst[t] = the sum over t's contiguous dz_em segment and dL/da_dst = sum_t g_s_dst[t] h[t]; adding
// g_s_dst[s] a_dst to g_h[s] is left to whoever reads g_h next.
// EN (round 6): the ENGINE's launches -- probabilities edge-major, no stamp buffer, a level of at least two edges, the source-order
// attribute copy at hand (single-attribute class), dz wanted in original edge order only (stored-term class) -- make those run-time
// flags compile-time constants (one_kind_en() on the host checks exactly that): the tests of uniform flags inside the row loop were
// part of the third of this kernel's issue slots that is scalar bookkeeping (profiles/r06_isa_mix.md).
template <int H, int KL, int RB, bool DF = false, bool EN = false>
__device__ __forceinline__ void gat_bwd_one_rows(const GatBwdOneArgs& A, float (*sA)[2 * FN_D], float (*sP)[8][kWfLd], int blk0, int se,
                                                 int rows_per_hw, int bid) {
    const float* __restrict__ g_out = A.g_out;
    const float* __restrict__ h = A.h;
    const float* __restrict__ cdot = A.cdot;
    const float* __restrict__ g_s_dst = A.g_s_dst;
    const fn_edge_term& et = A.et;
    const fn_gat_plan& pl = A.pl;
    const float slope = A.slope;
    float* __restrict__ g_h = A.g_h;
    float* __restrict__ dz_sorted = A.dz_sorted;
    float* __restrict__ g_s_orig = A.g_s_orig;
    constexpr int LPH = 32 / H;
    constexpr int NE = KL ? KL : 1;
    constexpr int NG = (2 * LPH >= 12 && KL == 1) ? 12 : 8;      // rows gathered in one round trip (the single-attribute class = the bond graph)
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH, hw = threadIdx.x >> 5;
    const int m = (int)pl.m, n = (int)pl.n;
    const int K = KL ? et.K : 0;
    const bool pairs = EN ? true : m >= 2;
    const bool want_orig = KL == 0 && (EN || g_s_orig != nullptr), want_sorted = KL == 0 && !EN && dz_sorted != nullptr;
    const float4 ad = ld4(A.att + head * A.att_w + A.dst_off + j * 4);
    const float4 as = ld4(A.att + head * A.att_w + A.src_off + j * 4);
    // signed probability of the edge at destination-order position q: p_head[q * p_step]
    const bool pem = EN ? true : A.p_edge_major != 0;
    const float* p_head = A.p_sorted + (pem ? (size_t)head : (size_t)head * m);
    const uint32_t p_step = pem ? 4u * H : 4u;                   // bytes
    // the source-order attribute copy is prefetched with the edge ids (two registers per attribute and row in flight): taken for the
    // single-attribute class only -- the wide class (fragment-bond graph: a small level) gathers from x_sorted instead
    constexpr int NX = KL == 1 ? 1 : 0;
    const bool xs = NX != 0 && (EN || A.x_src != nullptr);
    float4 qd = make_float4(0.f, 0.f, 0.f, 0.f), qs = qd;
    float pw[NE + 1];
#pragma unroll
    for (int k = 0; k <= NE; ++k) pw[k] = 0.f;
    const int sb = blk0 + hw;
    const int nr = A.n_real ? *A.n_real : n;
    unsigned long long* stw = (!EN && A.stamps) ? A.stamps + ((size_t)bid * (RB / 2) + (threadIdx.x >> 6)) * 16 : nullptr;
    auto stamp = [&](int slot, bool drain) {
        if (stw) {
            if (drain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == 0 && slot < 16) stw[slot] = t;
        }
    };
    stamp(0, false);

    auto load_extent = [&](int s, int& beg, int& deg, float& gsd) {
        const int sc = s < n ? s : n - 1;
        const i32x2u rp = ldp(pl.rowptr_s + sc);
        beg = rp.x - pl.pos_base_s;
        deg = s < se ? (s < nr ? rp.y - rp.x : 0) : -1;
        gsd = DF ? 0.f : g_s_dst[(uint32_t)sc * H + head];
    };
    auto issue_edges = [&](int beg, OneRaw<NX>& r) {
        int pos = beg + 2 * j;
        pos = pos > m - 2 ? m - 2 : pos;
        pos = pos < 0 ? 0 : pos;
        r.pos = pos;
        if constexpr (NX != 0) { r.x[0].x = r.x[0].y = 0.f; }
        if (!pairs) { r.tp.x = r.tp.y = 0;  r.dq.x = r.dq.y = 0;  return; }
        r.tp = ldp(pl.dst_s + pos);
        r.dq = ldp(pl.dpos_s + pos);
        if constexpr (NX != 0) { if (xs) r.x[0] = ldp(A.x_src + pos); }
    };

    int beg, deg, beg_n, deg_n;
    float gsd, gsd_n;
    OneRaw<NX> raw, cur;
    load_extent(sb, beg, deg, gsd);
    issue_edges(beg, raw);
    load_extent(sb + RB, beg_n, deg_n, gsd_n);
    cur = raw;
    asm volatile("" ::"v"(beg_n), "v"(deg_n), "v"(gsd_n), "v"(cur.tp.x), "v"(cur.tp.y), "v"(cur.dq.x), "v"(cur.dq.y));
    stamp(1, true);
    int it = 0;
    for (int s = sb; s < sb + RB * rows_per_hw; s += RB, ++it) {
        const bool fast = pairs && deg >= 0 && deg <= 2 * LPH;
        const bool has0 = fast && 2 * j < deg, has1 = fast && 2 * j + 1 < deg;
        const bool shifted = beg + 2 * j != cur.pos;              // only the very last edge of the level
        const int sc = s < n ? s : n - 1;
        // (a lane without an edge gathers its own row and any valid edge slot: weight 0, see gat_fwd_rows)
        const int t0 = has0 ? (shifted ? cur.tp.y : cur.tp.x) : sc, t1 = has1 ? cur.tp.y : t0;
        const int d0 = shifted ? cur.dq.y : cur.dq.x, d1 = cur.dq.y;
        // one round trip: next row's edge ids, the row after's extent, this row's per-edge scalars, its own row and the gradient rows
        issue_edges(beg_n, raw);
        int beg_nn, deg_nn;
        float gsd_nn;
        load_extent(s + 2 * RB, beg_nn, deg_nn, gsd_nn);
        const float ps0 = ld1_off(p_head, (uint32_t)d0 * p_step), ps1 = ld1_off(p_head, (uint32_t)d1 * p_step);
        const float c0 = ld1_off(cdot, ((uint32_t)t0 * H + head) * 4), c1 = ld1_off(cdot, ((uint32_t)t1 * H + head) * 4);
        float xa[NE], xb[NE];
        if constexpr (KL != 0) {
            if (NX != 0 && xs) { xa[0] = shifted ? cur.x[0].y : cur.x[0].x;  xb[0] = cur.x[0].y; }
            else {
#pragma unroll
                for (int k = 0; k < NE; ++k) {
                    const float* xk = et.x_sorted + (size_t)(k < K ? k : K - 1) * m;
                    xa[k] = ld1_off(xk, (uint32_t)d0 * 4);
                    xb[k] = ld1_off(xk, (uint32_t)d1 * 4);
                }
            }
        }
        int eq0 = 0, eq1 = 0;
        if (want_orig) { eq0 = pl.eid_d[d0];  eq1 = pl.eid_d[d1]; }
        const float4 hr = ld4_off(h, (uint32_t)sc * (FN_D * 4) + lane * 16);
        // gradient rows in flight per half-wave: 4, 8 or NG (wave-uniform tiers).  NG = 12 covers the bond graph's degree classes (a
        // bond between two four-valent atoms has 12 in- and out-edges: 28 % of ESOL-shape rows have 10 or 12); rows beyond the tier take
        // a second, dependent round trip below
        const bool wide = __any(fast && deg > 4), wide2 = NG > 8 && __any(fast && deg > 8);
        const bool live = __any(!fast || deg > 0);        // false: neither row of the wave has an out-edge (padding, isolated nodes)
        float4 r0[NG];
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
                r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
            }
        }
        // (a tier at 6: 57 % of the bond graph's rows have six edges -- two loads less for the waves whose two rows stop there)
        const bool wide8 = __any(fast && deg > (A.tier6 ? 6 : 4));
        if (wide) {
#pragma unroll
            for (int i = 4; i < 6; ++i) {
                const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
                r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
            }
        }
        if (wide8) {
#pragma unroll
            for (int i = 6; i < 8; ++i) {
                const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
                r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
            }
        }
        if (wide2) {
#pragma unroll
            for (int i = 8; i < NG; ++i) {
                const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
                r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
            }
        }
        if (it < 4) { stamp(2 + 3 * it, false);  stamp(3 + 3 * it, true); }
        const float p0 = has0 ? fabsf(ps0) : 0.f, p1 = has1 ? fabsf(ps1) : 0.f;
        float dp0 = 0.f, dp1 = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float dsum = head_sum<LPH>(dot4(hr, r0[i]));
                if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
        }
        if (wide) {
#pragma unroll
            for (int i = 4; i < 6; ++i) {
                const float dsum = head_sum<LPH>(dot4(hr, r0[i]));
                if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
        }
        if (wide8) {
#pragma unroll
            for (int i = 6; i < 8; ++i) {
                const float dsum = head_sum<LPH>(dot4(hr, r0[i]));
                if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
        }
        if (wide2) {
#pragma unroll
            for (int i = 8; i < NG; ++i) {
                const float dsum = head_sum<LPH>(dot4(hr, r0[i]));
                if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
            }
        }
        const int cur_beg = beg, cur_deg = deg;
        const float cur_gsd = gsd;
        cur = raw;
        beg = beg_n;  deg = deg_n;  gsd = gsd_n;  beg_n = beg_nn;  deg_n = deg_nn;  gsd_n = gsd_nn;
        float gss = 0.f;
        if (fast) {
            for (int k0 = NG; k0 < cur_deg; k0 += 4) {            // out-degree NG + 1 .. 2*LPH
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + i;
                    const int tk = __shfl((i & 1) ? t1 : t0, k >> 1, LPH);
                    const float pk = __shfl((i & 1) ? p1 : p0, k >> 1, LPH);
                    const float4 row = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
                    const float dsum = head_sum<LPH>(dot4(hr, row));
                    if ((k >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                    fma4(acc, pk, row);
                }
            }
            const float dz0 = has0 ? p0 * (dp0 - c0) * ((__float_as_uint(ps0) >> 31) ? slope : 1.f) : 0.f;
            const float dz1 = has1 ? p1 * (dp1 - c1) * ((__float_as_uint(ps1) >> 31) ? slope : 1.f) : 0.f;
            gss = head_sum<LPH>(dz0 + dz1);
            if constexpr (DF) {
                if (has0) st1_off(A.dz_em, ((uint32_t)d0 * H + head) * 4u, dz0);
                if (has1) st1_off(A.dz_em, ((uint32_t)d1 * H + head) * 4u, dz1);
            }
            if (KL == 0) {
                if (want_sorted) {                                // dL/d(edge term) at the edge's destination-order slot, [H][m]
                    if (has0) st1_next(dz_sorted, ((uint32_t)head * (uint32_t)m + (uint32_t)d0) * 4u, dz0);
                    if (has1) st1_next(dz_sorted, ((uint32_t)head * (uint32_t)m + (uint32_t)d1) * 4u, dz1);
                }
                if (want_orig) {                                  // ... in ORIGINAL edge order, [m_real][H]
                    if (has0 && eq0 < pl.m_real) st1_next(g_s_orig, ((uint32_t)eq0 * H + head) * 4u, dz0);
                    if (has1 && eq1 < pl.m_real) st1_next(g_s_orig, ((uint32_t)eq1 * H + head) * 4u, dz1);
                }
            } else {
                pw[NE] += dz0 + dz1;
#pragma unroll
                for (int k = 0; k < NE; ++k) pw[k] = fmaf(dz0, xa[k], fmaf(dz1, xb[k], pw[k]));
            }
            (void)xa;  (void)xb;
        } else if (cur_deg >= 0) {
            // rare high out-degree node (or a level with a single edge): every lane walks the edge list
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = 0; i < cur_deg; ++i) {
                const int pos = cur_beg + i;
                const int t = pl.dst_s[pos], dq = pl.dpos_s[pos];
                const float ps = ld1_off(p_head, (uint32_t)dq * p_step);
                const float cc = cdot[(size_t)t * H + head];
                const float4 row = ld4(g_out + (size_t)t * FN_D + lane * 4);
                const float dsum = head_sum<LPH>(dot4(hr, row));
                const float p = fabsf(ps);
                const float dz = p * (dsum - cc) * ((__float_as_uint(ps) >> 31) ? slope : 1.f);
                fma4(acc, p, row);
                gss += dz;
                if (j == 0) {
                    if constexpr (DF) A.dz_em[(size_t)dq * H + head] = dz;
                    if (KL == 0) {
                        if (want_sorted) dz_sorted[(size_t)head * m + dq] = dz;
                        if (want_orig) { const int eid = pl.eid_d[dq];  if (eid < pl.m_real) g_s_orig[(size_t)eid * H + head] = dz; }
                    } else {
                        pw[NE] += dz;
#pragma unroll
                        for (int kk = 0; kk < NE; ++kk)
                            if (kk < K) pw[kk] = fmaf(dz, et.x_sorted[(size_t)kk * m + dq], pw[kk]);
                    }
                }
            }
        }
        if (cur_deg >= 0 && s >= nr) {
            // padding row of a static-shape batch: its gradient is exactly 0 (and its h row / its dots were never written)
            st4_off(g_h, (uint32_t)s * (FN_D * 4) + lane * 16, make_float4(0.f, 0.f, 0.f, 0.f));
        } else if (cur_deg >= 0) {
            // (storing the row one iteration late, behind the next row's gathers, measured SLOWER: 18.5 -> 20.0 us at B = 512)
            if constexpr (!DF) fma4(acc, cur_gsd, ad);
            fma4(acc, gss, as);
            st4_next(g_h, (uint32_t)s * (FN_D * 4) + lane * 16, acc);        // the product launch behind this one reads it (store policy: fn_internal.h)
            if constexpr (!DF) fma4(qd, cur_gsd, hr);
            fma4(qs, gss, hr);
        }
        if (it < 4) stamp(4 + 3 * it, false);
    }
    stamp(14, false);
    st4(&sA[hw][lane * 4], qd);
    st4(&sA[hw][FN_D + lane * 4], qs);
    if (KL) {
#pragma unroll
        for (int k = 0; k <= NE; ++k) {
            const float v = head_sum<LPH>(pw[k]);
            if (j == 0) sP[hw][head][k == NE ? FN_MAX_EDGE_K : k] = v;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * FN_D; c += blockDim.x) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < RB; ++w) a += sA[w][c];
        A.part_a[part_at(A.part_ld, bid, c)] = a;           // (row-major, the engine's tables: consecutive threads, consecutive words)
    }
    if (KL) {
        // deterministic block partial of sum_e dz[e,h] * (x[e,0..K), 1); columns k >= K carry weight-0 duplicates
        const int ne = H * (K + 1);
        for (int i = threadIdx.x; i < ne; i += blockDim.x) {
            const int hh = i / (K + 1), k = i % (K + 1);
            const int kk = (k == K) ? FN_MAX_EDGE_K : k;
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < RB; ++w) a += sP[w][hh][kk];
            A.part_e[(size_t)bid * ne + i] = a;
        }
    }
    stamp(15, true);
}

template <int H, int KL, int RB, bool DF = false, bool EN = false>
__device__ __forceinline__ void gat_bwd_one_body(const GatBwdOneArgs& A, float (*sA)[2 * FN_D], float (*sP)[8][kWfLd], int bid, int nblk) {
    const int n = (int)A.pl.n, per = RB * A.rows_per_hw;                                // rows interleaved over the half-waves
    const int nr = A.n_real ? *A.n_real : n;
    const int blk0 = xcd_block_real(bid, nblk, A.n_real ? (nr + per - 1) / per : nblk) * per;      // real rows dealt evenly over the XCDs
    if (FN_PAD_BLOCK_EXIT && blk0 >= nr && !A.stamps) {
        // a workgroup whose rows are all padding (8-16 % of a static-shape batch's bond rows: the slack that hosts its padded edges):
        // zero gradient rows and zero partial sums, without the two dependent round trips and the row loop of the pipeline
        const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5, end = blk0 + per < n ? blk0 + per : n;
        for (int s = blk0 + hw; s < end; s += RB) st4(A.g_h + (size_t)s * FN_D + lane * 4, make_float4(0.f, 0.f, 0.f, 0.f));
        for (int c = threadIdx.x; c < 2 * FN_D; c += blockDim.x) A.part_a[part_at(A.part_ld, bid, c)] = 0.f;
        if (KL) {
            const int ne = H * (A.et.K + 1);
            for (int i = threadIdx.x; i < ne; i += blockDim.x) A.part_e[(size_t)bid * ne + i] = 0.f;
        }
        return;
    }
    gat_bwd_one_rows<H, KL, RB, DF, EN>(A, sA, sP, blk0, blk0 + per < n ? blk0 + per : n, A.rows_per_hw, bid);
}
template <int H, int KL, int RB, bool DF = false, bool EN = false>
__global__ __launch_bounds__(RB * 32, 3) void k_gat_bwd_one(GatBwdOneArgs A) {
    __shared__ float sA[RB][2 * FN_D];
    __shared__ float sP[RB][8][kWfLd];
    gat_bwd_one_body<H, KL, RB, DF, EN>(A, sA, sP, (int)blockIdx.x, (int)gridDim.x);
}
// the three levels whose gradients are complete at the same point of the backward pass -- bond graph (single attribute), atom graph
// (stored edge term), fragment-bond graph (K <= FN_MAX_EDGE_K attributes) -- in one launch; a level with nblk == 0 is absent
template <int H, int RB, bool EN = false>
__global__ __launch_bounds__(RB * 32, 3) void k_gat_bwd_one3(GatBwdOneArgs A, GatBwdOneArgs B, GatBwdOneArgs C, int interleave) {
    __shared__ float sA[RB][2 * FN_D];
    __shared__ float sP[RB][8][kWfLd];
    // block order: the bond level's workgroups ALTERNATE with the others' (atom level, then fragment-bond level) as long as both
    // kinds last, so that every CU hosts both from the first round on (level after level, the launch took the sum of the levels'
    // stand-alone times: each is bound by its own dependent round trips and leaves the CU idle in between)
    const int nX = A.nblk, nY = B.nblk + C.nblk, mn = nX < nY ? nX : nY;
    int b = (int)blockIdx.x, g;
    if (interleave && b < 2 * mn) { g = b & 1;  b >>= 1; }
    else if (interleave) { g = nX > nY ? 0 : 1;  b -= mn; }
    else { g = b < nX ? 0 : 1;  b -= g ? nX : 0; }
    if (g == 0) gat_bwd_one_body<H, 1, RB, false, EN>(A, sA, sP, b, A.nblk);
    else if (b < B.nblk) gat_bwd_one_body<H, 0, RB, false, EN>(B, sA, sP, b, B.nblk);
    else gat_bwd_one_body<H, FN_MAX_EDGE_K, RB, false, EN>(C, sA, sP, b - B.nblk, C.nblk);
}

// c[t, h] = scale <g[t, h, :], out[t, h, :]>,  u[t, h] = <g[t, h, :], out2[t, h, :]> - c[t, h] sigma[t, h]: the two node-local
// dots the one-pass backward needs, for gradient rows whose producer cannot form them (the last layer's, and the per-level
// operator path); inner layers get them from the input-gradient GEMM's epilogue (CuEpi).  `out` may be the level's
// relu(dropout(.)) output y with scale = 1 - p when g flows through that gate only (g is 0 wherever y is, and y = out / (1 - p)
// wherever it is not).
using fni::CuTask;
using fni::CuTasks;
template <int H>
__global__ __launch_bounds__(kBlock) void k_gat_cu(CuTasks T) {
    constexpr int LPH = 32 / H;
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const CuTask& t = T.t[ti];
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH;
    const int b = (int)blockIdx.x - t.first;
    for (int64_t r = (int64_t)b * kRows + (threadIdx.x >> 5); r < t.n; r += (int64_t)t.nblk * kRows) {
        const float4 g = ld4(t.g + r * FN_D + lane * 4);
        const float4 o = ld4(t.out + r * FN_D + lane * 4);
        const float c = t.scale * head_sum<LPH>(dot4(g, o));
        if (t.out2) {        // (null: only c is wanted -- the operator-level deferred form, DF above)
            const float4 o2 = ld4(t.out2 + r * FN_D + lane * 4);
            const float sg = t.sigma[r * H + head];
            const float u = head_sum<LPH>(dot4(g, o2)) - c * sg;
            if (j == 0) t.u[r * H + head] = u;
        }
        if (j == 0) t.c[r * H + head] = c;
    }
}

// g_s_dst[t, 0..4) = the sum of row t's contiguous dz_em segment, behind a deferred pass (DF above; fn_gat_gsd_f32 -- operator level,
// the engine does not launch it).  Sixteen lanes per row, lane i adds the floats (beg + 4 j) * 4 + i, two row rotations add the four
// parts -- every lane then holds the sum of head i & 3.  The same lanes also take the level's dL/da_dst = sum_t g_s_dst[t, h] h[t, head h's columns]
// (lane i: the eight columns 32 (i & 3) + 8 (i >> 2) .. of its row): the pass itself left zeros in those columns of part_a, this
// kernel overwrites them -- one row of partial sums per block, as many blocks as the pass had (the deferred reduction adds n_a rows).
using fni::GsdSegTask;
using fni::GsdSegTasks;
__global__ __launch_bounds__(kBlock) void k_gsd_seg(GsdSegTasks T) {
    __shared__ float sQ[kBlock / 16][FN_D];
    int ti = 0;
    while (ti + 1 < T.n && (int)blockIdx.x >= T.t[ti + 1].first) ++ti;
    const GsdSegTask& t = T.t[ti];
    const int i = threadIdx.x & 15, part = i >> 2, rg = threadIdx.x >> 4, b = (int)blockIdx.x - t.first;
    const int64_t nr = t.n_real ? (int64_t)*t.n_real : t.n;
    const int64_t per = (t.n + t.nblk - 1) / t.nblk, r_end = (b + 1) * per < t.n ? (b + 1) * per : t.n;
    const int c0 = 32 * (i & 3) + 8 * part;
    float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
    for (int64_t row = (int64_t)b * per + rg; row < r_end; row += kBlock / 16) {
        const int beg = t.rowptr[row] - t.pos_base;
        const int deg = row < nr ? t.rowptr[row + 1] - t.rowptr[row] : 0;
        const float4 h0 = deg > 0 ? ld4(t.h + row * FN_D + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 h1 = deg > 0 ? ld4(t.h + row * FN_D + c0 + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        float a = 0.f;
        for (int jj = 0; __any(part + 4 * jj < deg); ++jj) {
            const bool ok = part + 4 * jj < deg;
            const float x = ld1_off(t.dz + i, ok ? (uint32_t)(beg + 4 * jj) * 16u : 0u);
            a += ok ? x : 0.f;
        }
        a += dpp_mov<0x128>(a);       // row_ror:8
        a += dpp_mov<0x124>(a);       // row_ror:4
        if (part == 0) t.gsd[row * 4 + i] = a;
        fma4(q0, a, h0);
        fma4(q1, a, h1);
    }
    st4(&sQ[rg][c0], q0);
    st4(&sQ[rg][c0 + 4], q1);
    __syncthreads();
    if (threadIdx.x < FN_D) {
        float v = 0.f;
#pragma unroll
        for (int g = 0; g < kBlock / 16; ++g) v += sQ[g][threadIdx.x];
        t.part_a[(size_t)threadIdx.x * FN_MAX_PART + b] = v;
    }
}
