// gat_bwd_two.inc -- the general TWO-PASS backward of an attention level (destination pass + source pass; rounds 1-3) and the
// by-source attention read-out (k_attn_by_src): device code and the host-side argument preparation, included inside the anonymous
// namespace of fragnet_hip.hip (the destination pass, k_attn_by_src) and of encoder.hip (the source pass and the combined
// launches that run the same bodies)
// behind gat_fwd.inc.  Templates and inline functions only: a __global__ function that is no template would be compiled into both
// units.  (The finalize of the partials these passes write, gat_finalize_body with k_gat_finalize, is in param_grads.hip, beside
// k_reduce_tasks.)  The engine's default since round 4 is the one-pass backward (gat_bwd_one.inc); these kernels serve head counts and
// hand-built graphs the one-pass kernel does not take, the fragment graph inside the tail (mol_tail.inc shares their row cores) and
// the operator path's fallback (fn_gat_bwd_dst_f32 / fn_gat_bwd_src_f32).

// Backward kernels use RB rows (half-waves) per block.
// Destination pass: dz[e] = p[e] * (<g_out[dst], h[src]> - sum_e' p[e'] <g_out[dst], h[src']>) * LeakyReLU', per head.
// Same shape as the forward kernel: persistent half-waves over R consecutive rows, straight-line body with clamped
// unconditional loads, the next row's edge data fetched while this row's source rows fly.
template <int NE> struct BwdRaw {
    int pos;
    i32x2u sp, sq, eq;        // source ids, positions in source order, original edge ids
    f32x2u pp;                // signed probabilities
    f32x2u x[NE];             // raw edge attributes (mode 2)
};

struct GatBwdDstArgs {
    const float *g_out, *h, *p_sorted;
    fn_edge_term et;
    fn_gat_plan pl;
    float slope;
    float *dz_sorted, *g_s_orig, *pz_src, *g_s_dst, *part_e;
    int rows_per_hw, nblk;
};
// rows [blk0, te) interleaved over the block's RB half-waves; bid: the block's slot in part_e (KL != 0)
template <int H, int KL, int RB>
__device__ __forceinline__ void gat_bwd_dst_rows(const GatBwdDstArgs& A, float (*sP)[8][kWfLd], int blk0, int te, int rows_per_hw, int bid) {
    const float* __restrict__ g_out = A.g_out;
    const float* __restrict__ h = A.h;
    const float* __restrict__ p_sorted = A.p_sorted;
    const fn_edge_term& et = A.et;
    const fn_gat_plan& pl = A.pl;
    const float slope = A.slope;
    float* __restrict__ dz_sorted = A.dz_sorted;
    float* __restrict__ g_s_orig = A.g_s_orig;
    float* __restrict__ pz_src = A.pz_src;
    float* __restrict__ g_s_dst = A.g_s_dst;
    float* __restrict__ part_e = A.part_e;
    constexpr int LPH = 32 / H;
    constexpr int NE = KL ? KL : 1;
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH, hw = threadIdx.x >> 5;
    const int m = (int)pl.m, n = (int)pl.n;
    const int K = KL ? et.K : 0;
    const bool pairs = m >= 2;
    const bool want_orig = KL == 0 && g_s_orig != nullptr;
    float pw[NE + 1];
#pragma unroll
    for (int k = 0; k <= NE; ++k) pw[k] = 0.f;
    const float* p_head = p_sorted + (size_t)head * m;
    float* pz_head = pz_src + (size_t)head * m * 2;
    const int tb = blk0 + hw;

    auto load_extent = [&](int t, int& beg, int& deg) {
        const int tc = t < n ? t : n - 1;
        const i32x2u rp = ldp(pl.rowptr_d + tc);
        beg = rp.x - pl.pos_base_d;
        deg = t < te ? rp.y - rp.x : -1;
    };
    auto issue_edges = [&](int beg, BwdRaw<NE>& r) {
        int pos = beg + 2 * j;
        pos = pos > m - 2 ? m - 2 : pos;
        pos = pos < 0 ? 0 : pos;
        r.pos = pos;
        if (!pairs) { r.sp.x = r.sp.y = 0;  r.sq.x = r.sq.y = 0;  r.eq.x = r.eq.y = 0;  r.pp.x = r.pp.y = 0.f;  return; }
        r.sp = ldp(pl.src_d + pos);
        r.pp = ldp(p_head + pos);
        r.sq = ldp(pl.spos_d + pos);
        if (want_orig) r.eq = ldp(pl.eid_d + pos);
        if (KL) {
#pragma unroll
            for (int k = 0; k < NE; ++k) r.x[k] = ldp(et.x_sorted + (size_t)(k < K ? k : K - 1) * m + pos);
        }
    };

    int beg, deg, beg_n, deg_n;
    BwdRaw<NE> raw, cur;
    load_extent(tb, beg, deg);
    issue_edges(beg, raw);
    load_extent(tb + RB, beg_n, deg_n);
    cur = raw;
    asm volatile("" ::"v"(beg_n), "v"(deg_n), "v"(cur.sp.x), "v"(cur.sp.y), "v"(cur.pp.x), "v"(cur.pp.y), "v"(cur.sq.x), "v"(cur.sq.y));
    for (int t = tb; t < tb + RB * rows_per_hw; t += RB) {
        const bool fast = pairs && deg >= 0 && deg <= 2 * LPH;
        const bool has0 = fast && 2 * j < deg, has1 = fast && 2 * j + 1 < deg;
        const bool shifted = beg + 2 * j != cur.pos;              // only the very last edge of the level
        // (a lane without an edge gathers the destination row itself, see gat_fwd_rows)
        const int src0 = has0 ? (shifted ? cur.sp.y : cur.sp.x) : (t < n ? t : n - 1), src1 = has1 ? cur.sp.y : src0;
        const float ps0 = has0 ? (shifted ? cur.pp.y : cur.pp.x) : 0.f, ps1 = has1 ? cur.pp.y : 0.f;
        const int sq0 = shifted ? cur.sq.y : cur.sq.x, sq1 = cur.sq.y;
        const int eq0 = shifted ? cur.eq.y : cur.eq.x, eq1 = cur.eq.y;
        // one round trip: next row's edge data, the row after's extent, this row's gradient row and source rows
        issue_edges(beg_n, raw);
        int beg_nn, deg_nn;
        load_extent(t + 2 * RB, beg_nn, deg_nn);
        const int tc = t < n ? t : n - 1;
        const float4 g = ld4_off(g_out, (uint32_t)tc * (FN_D * 4) + lane * 16);
        const bool wide = __any(fast && deg > 4);
        float4 r0[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
            r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
        }
        if (wide) {
#pragma unroll
            for (int i = 4; i < 8; ++i) {
                const int sk = __shfl((i & 1) ? src1 : src0, i >> 1, LPH);
                r0[i] = ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16);
            }
        }
        float dp0 = 0.f, dp1 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dsum = head_sum<LPH>(dot4(g, r0[i]));
            if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
        }
        if (wide) {
#pragma unroll
            for (int i = 4; i < 8; ++i) {
                const float dsum = head_sum<LPH>(dot4(g, r0[i]));
                if ((i >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
            }
        }
        if (fast) {
            for (int k0 = 8; k0 < deg; k0 += 4) {                 // in-degree 9 .. 2*LPH
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + i;
                    const int sk = __shfl((i & 1) ? src1 : src0, k >> 1, LPH);
                    const float dsum = head_sum<LPH>(dot4(g, ld4_off(h, (uint32_t)sk * (FN_D * 4) + lane * 16)));
                    if ((k >> 1) == j) { if (i & 1) dp1 = dsum; else dp0 = dsum; }
                }
            }
        }
        const float p0 = fabsf(ps0), p1 = fabsf(ps1);
        const float c = head_sum<LPH>(p0 * dp0 + p1 * dp1);
        const float dz0 = p0 * (dp0 - c) * ((__float_as_uint(ps0) >> 31) ? slope : 1.f);
        const float dz1 = p1 * (dp1 - c) * ((__float_as_uint(ps1) >> 31) ? slope : 1.f);
        // the raw data of this row is consumed: take over the next row's before the stores (see k_gat_fwd)
        float xa[NE], xb[NE];
#pragma unroll
        for (int k = 0; k < NE; ++k) { xa[k] = shifted ? cur.x[k].y : cur.x[k].x;  xb[k] = cur.x[k].y; }
        const int pos0 = beg + 2 * j, t_cur_deg = deg, t_cur_beg = beg;
        cur = raw;
        beg = beg_n;  deg = deg_n;  beg_n = beg_nn;  deg_n = deg_nn;
        if (fast) {
            if (has0) stp(pz_head + (size_t)sq0 * 2, p0, dz0);
            if (has1) stp(pz_head + (size_t)sq1 * 2, p1, dz1);
            if (KL == 0) {
                if (dz_sorted) {
                    if (has1) stp(dz_sorted + (size_t)head * m + pos0, dz0, dz1);
                    else if (has0) dz_sorted[(size_t)head * m + pos0] = dz0;
                }
                if (want_orig) {                                  // gradient of the edge term in ORIGINAL edge order, [m_real][H]
                    if (has0 && eq0 < pl.m_real) g_s_orig[(size_t)eq0 * H + head] = dz0;
                    if (has1 && eq1 < pl.m_real) g_s_orig[(size_t)eq1 * H + head] = dz1;
                }
            } else {
                pw[NE] += dz0 + dz1;                              // dz is 0 where the lane has no edge
#pragma unroll
                for (int k = 0; k < NE; ++k) pw[k] = fmaf(dz0, xa[k], fmaf(dz1, xb[k], pw[k]));
            }
            const float gs = head_sum<LPH>(dz0 + dz1);
            if (j == 0) g_s_dst[(size_t)t * H + head] = gs;
        } else if (t_cur_deg >= 0) {
            // rare high in-degree node (or a level with a single edge): every lane walks the edge list
            const int bg = t_cur_beg, dg = t_cur_deg;
            float cs = 0.f;
            for (int k = 0; k < dg; ++k) {
                const int sk = pl.src_d[bg + k];
                const float dsum = head_sum<LPH>(dot4(g, ld4(h + (size_t)sk * FN_D + lane * 4)));
                cs = fmaf(fabsf(p_head[bg + k]), dsum, cs);
            }
            float gs = 0.f;
            for (int k = 0; k < dg; ++k) {
                const int sk = pl.src_d[bg + k];
                const float dsum = head_sum<LPH>(dot4(g, ld4(h + (size_t)sk * FN_D + lane * 4)));
                const float ps = p_head[bg + k];
                const float dz = fabsf(ps) * (dsum - cs) * ((__float_as_uint(ps) >> 31) ? slope : 1.f);
                if (j == 0) {
                    stp(pz_head + (size_t)pl.spos_d[bg + k] * 2, fabsf(ps), dz);
                    if (KL == 0) {
                        if (dz_sorted) dz_sorted[(size_t)head * m + bg + k] = dz;
                        if (g_s_orig) { const int eid = pl.eid_d[bg + k]; if (eid < pl.m_real) g_s_orig[(size_t)eid * H + head] = dz; }
                    } else {
                        pw[NE] += dz;
#pragma unroll
                        for (int kk = 0; kk < NE; ++kk)
                            if (kk < K) pw[kk] = fmaf(dz, et.x_sorted[(size_t)kk * m + bg + k], pw[kk]);
                    }
                }
                gs += dz;
            }
            if (j == 0) g_s_dst[(size_t)t * H + head] = gs;
        }
    }

    if (KL) {
        // deterministic block partial of sum_e dz[e,h] * (x[e,0..K), 1); columns k >= K carry weight-0 duplicates
#pragma unroll
        for (int k = 0; k <= NE; ++k) {
            const float v = head_sum<LPH>(pw[k]);
            if (j == 0) sP[hw][head][k == NE ? FN_MAX_EDGE_K : k] = v;
        }
        __syncthreads();
        const int ne = H * (K + 1);
        for (int i = threadIdx.x; i < ne; i += blockDim.x) {
            const int hh = i / (K + 1), k = i % (K + 1);
            const int kk = (k == K) ? FN_MAX_EDGE_K : k;
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < RB; ++w) a += sP[w][hh][kk];
            part_e[(size_t)bid * ne + i] = a;
        }
    }
}

// Source pass: g_h[s] = sum over out-edges p * g_out[dst] + g_s_dst[s] * a_dst + (sum dz) * a_src, and the block
// partials of dL/da_dst, dL/da_src.  Its stores are whole rows, so it pipelines like the forward kernel: persistent
// half-waves over R consecutive source rows, straight-line body, next row's (dst ids, p, dz) in flight during the
// gathers of this one.
struct SrcRaw {
    int pos;
    i32x2u tp;
    f32x4u v;               // p0, dz0, p1, dz1
};

template <int H, int KL, int RB>
__device__ __forceinline__ void gat_bwd_dst_body(const GatBwdDstArgs& A, float (*sP)[8][kWfLd], int bid, int nblk) {
    const int blk0 = xcd_block(bid, nblk) * RB * A.rows_per_hw, n = (int)A.pl.n;      // rows interleaved over the half-waves
    gat_bwd_dst_rows<H, KL, RB>(A, sP, blk0, blk0 + RB * A.rows_per_hw < n ? blk0 + RB * A.rows_per_hw : n, A.rows_per_hw, bid);
}
template <int H, int KL, int RB>
__global__ __launch_bounds__(RB * 32) void k_gat_bwd_dst(GatBwdDstArgs A) {
    __shared__ float sP[RB][8][kWfLd];
    gat_bwd_dst_body<H, KL, RB>(A, sP, (int)blockIdx.x, (int)gridDim.x);
}

struct GatBwdSrcArgs {
    const float *g_out, *h, *pz_src, *g_s_dst, *att;
    int att_w, dst_off, src_off;
    fn_gat_plan pl;
    float *g_h, *part_a;
    int rows_per_hw, nblk;
    int part_ld;              // layout of part_a (part_at, fn_internal.h): 0 = column-major [256][FN_MAX_PART], else row-major [nblk][part_ld]
};
// source rows [blk0, se) interleaved over the block's RB half-waves; bid: the block's slot (row) in part_a
template <int H, int RB>
__device__ __forceinline__ void gat_bwd_src_rows(const GatBwdSrcArgs& A, float (*sA)[2 * FN_D], int blk0, int se, int rows_per_hw, int bid) {
    const float* __restrict__ g_out = A.g_out;
    const float* __restrict__ h = A.h;
    const float* __restrict__ pz_src = A.pz_src;
    const float* __restrict__ g_s_dst = A.g_s_dst;
    const float* __restrict__ att = A.att;
    const int att_w = A.att_w, dst_off = A.dst_off, src_off = A.src_off;
    const fn_gat_plan& pl = A.pl;
    float* __restrict__ g_h = A.g_h;
    float* __restrict__ part_a = A.part_a;
    constexpr int LPH = 32 / H;
    const int lane = threadIdx.x & 31, head = lane / LPH, j = lane % LPH, hw = threadIdx.x >> 5;
    const int m = (int)pl.m, n = (int)pl.n;
    const bool pairs = m >= 2;
    const float4 ad = ld4(att + head * att_w + dst_off + j * 4);
    const float4 as = ld4(att + head * att_w + src_off + j * 4);
    const float* pz_head = pz_src + (size_t)head * m * 2;
    float4 qd = make_float4(0.f, 0.f, 0.f, 0.f), qs = qd;
    const int sb = blk0 + hw;

    auto load_extent = [&](int s, int& beg, int& deg, float& gsd) {
        const int sc = s < n ? s : n - 1;
        const i32x2u rp = ldp(pl.rowptr_s + sc);
        beg = rp.x - pl.pos_base_s;
        deg = s < se ? rp.y - rp.x : -1;
        gsd = g_s_dst[(uint32_t)sc * H + head];
    };
    auto issue_edges = [&](int beg, SrcRaw& r) {
        int pos = beg + 2 * j;
        pos = pos > m - 2 ? m - 2 : pos;
        pos = pos < 0 ? 0 : pos;
        r.pos = pos;
        if (!pairs) { r.tp.x = r.tp.y = 0;  r.v.x = r.v.y = r.v.z = r.v.w = 0.f;  return; }
        r.tp = ldp(pl.dst_s + pos);
        r.v = *reinterpret_cast<const f32x4u*>(pz_head + (size_t)pos * 2);
    };

    int beg, deg, beg_n, deg_n;
    float gsd, gsd_n;
    SrcRaw raw, cur;
    load_extent(sb, beg, deg, gsd);
    issue_edges(beg, raw);
    load_extent(sb + RB, beg_n, deg_n, gsd_n);
    cur = raw;
    asm volatile("" ::"v"(beg_n), "v"(deg_n), "v"(gsd_n), "v"(cur.tp.x), "v"(cur.tp.y), "v"(cur.v.x), "v"(cur.v.y), "v"(cur.v.z), "v"(cur.v.w));
    for (int s = sb; s < sb + RB * rows_per_hw; s += RB) {
        const bool fast = pairs && deg >= 0 && deg <= 2 * LPH;
        const bool has0 = fast && 2 * j < deg, has1 = fast && 2 * j + 1 < deg;
        const bool shifted = beg + 2 * j != cur.pos;              // only the very last edge of the level
        const int t0 = has0 ? (shifted ? cur.tp.y : cur.tp.x) : (s < n ? s : n - 1), t1 = has1 ? cur.tp.y : t0;      // (no edge: the row itself)
        const float p0 = has0 ? (shifted ? cur.v.z : cur.v.x) : 0.f, z0 = has0 ? (shifted ? cur.v.w : cur.v.y) : 0.f;
        const float p1 = has1 ? cur.v.z : 0.f, z1 = has1 ? cur.v.w : 0.f;
        issue_edges(beg_n, raw);
        int beg_nn, deg_nn;
        float gsd_nn;
        load_extent(s + 2 * RB, beg_nn, deg_nn, gsd_nn);
        const int sc = s < n ? s : n - 1;
        const float4 hr = ld4_off(h, (uint32_t)sc * (FN_D * 4) + lane * 16);
        const bool wide = __any(fast && deg > 4);
        float4 r0[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
            r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
        }
        if (wide) {
#pragma unroll
            for (int i = 4; i < 8; ++i) {
                const int tk = __shfl((i & 1) ? t1 : t0, i >> 1, LPH);
                r0[i] = ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16);
            }
        }
        float gss = head_sum<LPH>(z0 + z1);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
        if (wide) {
#pragma unroll
            for (int i = 4; i < 8; ++i) fma4(acc, __shfl((i & 1) ? p1 : p0, i >> 1, LPH), r0[i]);
        }
        const int cur_beg = beg, cur_deg = deg;
        const float cur_gsd = gsd;
        cur = raw;
        beg = beg_n;  deg = deg_n;  gsd = gsd_n;  beg_n = beg_nn;  deg_n = deg_nn;  gsd_n = gsd_nn;
        if (fast) {
            for (int k0 = 8; k0 < cur_deg; k0 += 4) {             // out-degree 9 .. 2*LPH
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = k0 + i;
                    const int tk = __shfl((i & 1) ? t1 : t0, k >> 1, LPH);
                    const float pk = __shfl((i & 1) ? p1 : p0, k >> 1, LPH);
                    fma4(acc, pk, ld4_off(g_out, (uint32_t)tk * (FN_D * 4) + lane * 16));
                }
            }
        } else if (cur_deg >= 0) {
            acc = make_float4(0.f, 0.f, 0.f, 0.f);
            gss = 0.f;
            for (int i = 0; i < cur_deg; ++i) {
                const int t = pl.dst_s[cur_beg + i];
                const f32x2u v = ldp(pz_head + (size_t)(cur_beg + i) * 2);
                fma4(acc, v.x, ld4(g_out + (size_t)t * FN_D + lane * 4));
                gss += v.y;
            }
        }
        if (cur_deg >= 0) {
            fma4(acc, cur_gsd, ad);
            fma4(acc, gss, as);
            st4(g_h + (size_t)s * FN_D + lane * 4, acc);
            fma4(qd, cur_gsd, hr);
            fma4(qs, gss, hr);
        }
    }
    st4(&sA[hw][lane * 4], qd);
    st4(&sA[hw][FN_D + lane * 4], qs);
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * FN_D; c += blockDim.x) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < RB; ++w) a += sA[w][c];
        part_a[part_at(A.part_ld, bid, c)] = a;
    }
}

template <int H, int RB>
__device__ __forceinline__ void gat_bwd_src_body(const GatBwdSrcArgs& A, float (*sA)[2 * FN_D], int bid, int nblk) {
    const int blk0 = xcd_block(bid, nblk) * RB * A.rows_per_hw, n = (int)A.pl.n;      // rows interleaved over the half-waves
    gat_bwd_src_rows<H, RB>(A, sA, blk0, blk0 + RB * A.rows_per_hw < n ? blk0 + RB * A.rows_per_hw : n, A.rows_per_hw, bid);
}
template <int H, int RB>
__global__ __launch_bounds__(RB * 32) void k_gat_bwd_src(GatBwdSrcArgs A) {
    __shared__ float sA[RB][2 * FN_D];
    gat_bwd_src_body<H, RB>(A, sA, (int)blockIdx.x, (int)gridDim.x);
}


template <int H>
__global__ void k_attn_by_src(const float* __restrict__ p_sorted, fn_gat_plan pl, float* __restrict__ attn) {
    const int64_t total = pl.n * H;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / H;
        const int head = (int)(i % H);
        const int beg = pl.rowptr_s[s] - pl.pos_base_s, deg = pl.rowptr_s[s + 1] - pl.rowptr_s[s];
        float a = 0.f;
        for (int k = 0; k < deg; ++k) a += fabsf(p_sorted[(size_t)head * pl.m + pl.dpos_s[beg + k]]);
        attn[i] = a;
    }
}

// ---- host side: argument validation + launch geometry of the two passes (shared by the single-level C-ABI entry points in
// fragnet_hip.hip and the engine's combined launches in encoder.hip, which carry these argument blocks inside launches of their own:
// k_tail_bwd, k_gat_bwd_src_rd); nblk == 0 means "nothing to do"
inline int prep_gat_bwd_dst(const float* g_out, const float* h, const float* p_sorted, const fn_edge_term* et,
                            const fn_gat_plan* plan, float neg_slope, float* dz_sorted, float* g_s_orig, float* pz_src,
                            float* g_s_dst, float* part_e, int* n_part_e, int heads, GatBwdDstArgs* A) {
    if (!g_out || !h || !plan || !g_s_dst || !n_part_e || !et) return fni::fail(FN_EINVAL, "fn_gat_bwd_dst_f32: bad argument");
    if (et->mode != 0 && fni::bad_edge_term(et, plan ? plan->m : 1)) return fni::fail(FN_EINVAL, "fn_gat_bwd_dst_f32: bad edge term");
    if (plan->m > 0 && (!p_sorted || !pz_src || !plan->spos_d || (et->mode == 0 && !dz_sorted && !g_s_orig)))
        return fni::fail(FN_EINVAL, "fn_gat_bwd_dst_f32: null edge buffer");
    if (et->mode == 2 && !part_e) return fni::fail(FN_EINVAL, "fn_gat_bwd_dst_f32: null part_e");
    if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return fni::fail(FN_EUNSUPPORTED, "heads must be 1, 2, 4 or 8 (128 = heads * head_dim)");
    *n_part_e = 0;
    *A = GatBwdDstArgs{g_out, h, p_sorted, *et, *plan, neg_slope, dz_sorted, g_s_orig, pz_src, g_s_dst, part_e, 1, 0};
    if (plan->n == 0) return 0;
    if (plan->n > (1 << 23) || plan->m * heads > (1 << 29))
        return fni::fail(FN_EUNSUPPORTED, "fn_gat_bwd_dst_f32: level too large for 32-bit byte offsets (n <= 2^23 rows, m*heads <= 2^29)");
    // R rows per half-wave; one edge-parameter partial row per block, hence at most FN_MAX_PART blocks.
    // Unlike the forward kernel this one wants R SMALL: its (p, dz) stores are scattered 8-byte writes into source
    // order, vmcnt counts loads and stores in one in-order queue, so every extra row per wave waits behind the
    // previous row's slow stores (B=2048: R=4 56 us, R=8 84 us; B=512: 16 us at any R)
    const int64_t groups = (plan->n + kBwdRows - 1) / kBwdRows;
    // rows per half-wave: ~groups / 1536 (three at ESOL batch 512: 0.926 -> 0.902 ms per step against one row each), but at most
    // three -- the (p, dz) stores into source order are scattered and every further row waits behind them (B = 2048: 56 us at
    // four rows, 84 us at eight) -- unless the level is so large that the partial rows would not fit FN_MAX_PART
    const int64_t resident = fni::tune(FN_TUNE_DST_BLOCKS) > 0 && fni::tune(FN_TUNE_DST_BLOCKS) < FN_MAX_PART ? fni::tune(FN_TUNE_DST_BLOCKS) : FN_MAX_PART;
    const int64_t need = (groups + FN_MAX_PART - 1) / FN_MAX_PART, want = (groups + resident - 1) / resident;
    A->rows_per_hw = (int)std::max<int64_t>(need, std::min<int64_t>(want, 3));
    A->nblk = (int)((plan->n + (int64_t)kBwdRows * A->rows_per_hw - 1) / ((int64_t)kBwdRows * A->rows_per_hw));
    *n_part_e = (et->mode == 2) ? A->nblk : 0;
    return 0;
}

inline int prep_gat_bwd_src(const float* g_out, const float* h, const float* pz_src, const float* g_s_dst, const float* att,
                            int att_w, int dst_off, int src_off, const fn_gat_plan* plan, float* g_h, float* part_a,
                            int* n_part_a, int heads, GatBwdSrcArgs* A) {
    if (!g_out || !h || !g_s_dst || !att || !plan || !g_h || !part_a || !n_part_a) return fni::fail(FN_EINVAL, "fn_gat_bwd_src_f32: bad argument");
    if (plan->m > 0 && !pz_src) return fni::fail(FN_EINVAL, "fn_gat_bwd_src_f32: null edge buffer");
    if ((att_w | dst_off | src_off) & 3) return fni::fail(FN_EINVAL, "fn_gat_bwd_src_f32: att blocks must be 16-byte aligned");
    if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return fni::fail(FN_EUNSUPPORTED, "heads must be 1, 2, 4 or 8 (128 = heads * head_dim)");
    *n_part_a = 0;
    *A = GatBwdSrcArgs{g_out, h, pz_src, g_s_dst, att, att_w, dst_off, src_off, *plan, g_h, part_a, 1, 0};
    if (plan->n == 0) return 0;
    if (plan->n > (1 << 23) || plan->m * heads > (1 << 28))
        return fni::fail(FN_EUNSUPPORTED, "fn_gat_bwd_src_f32: level too large for 32-bit byte offsets (n <= 2^23 rows, m*heads <= 2^28)");
    // every block writes a row of 256 partial sums: at most 1024 blocks, each half-wave pipelining R rows
    const int64_t groups = (plan->n + kBwdRows - 1) / kBwdRows;
    int64_t resident = (int64_t)fni::tune(FN_TUNE_SRC_BLOCKS);
    if (resident > 1024 || resident < 1) resident = 1024;
    A->rows_per_hw = (int)((groups + resident - 1) / resident);
    A->nblk = (int)((plan->n + (int64_t)kBwdRows * A->rows_per_hw - 1) / ((int64_t)kBwdRows * A->rows_per_hw));
    *n_part_a = A->nblk;
    return 0;
}
