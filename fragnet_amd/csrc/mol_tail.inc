// Molecule-resident fragment tail of the encoder (included by encoder.hip, inside its anonymous namespace, behind gat_fwd.inc,
// gat_bwd_two.inc and the row-dots backward, whose row cores its global-memory path runs).
//
// The last layer's fragment levels are tiny per molecule (ESOL: 3.6 fragments, 6 fragment-graph edges, 26 atoms) and ran as a
// chain of small launches that each cost their latency floor (~5 us however little they do):
//   forward   atom -> fragment sum + node scalars + edge term (k_frag_tail) -> fragment-graph attention (k_gat_fwd) -> readout
//             (k_pool_cat)                                                                              3 launches, 17 us at B = 512
//   backward  readout backward (k_pool_cat_bwd) -> relu/dropout gates (k_gate_many) -> destination pass -> source pass + edge-term
//             backward -> scatter of dL/d(fragment sums) to the atoms (k_gather_rows4)                   5 launches, 30 us
// The graphs are block-diagonal per molecule (collate_fn concatenates molecules, dataset/data.py:877-948), so ONE workgroup per
// molecule can run the whole chain with workgroup barriers in place of kernel boundaries: k_tail_fwd / k_tail_bwd.
//  * LDS path (a molecule of <= kTailNF fragments and <= kTailME fragment-graph edges -- every molecule of the reference's
//    datasets): the molecule's slice of the plan, its fragment rows, per-edge probabilities and gradients live in LDS, so the
//    kernel makes three to four dependent global round trips (extents -> plan slice + rows -> gathered rows -> stores)
//    instead of the eleven of the chained launches; the per-edge loops are serial per head (a fragment has ~2 in-edges).
//  * global path (larger molecules): the phases are the row-range cores of the stand-alone kernels (gat_fwd_rows,
//    gat_bwd_dst_rows, gat_bwd_src_rows, row_dots_sorted_bwd_range) restricted to the molecule's rows; intermediate tensors go
//    through global memory (L2-resident, written and read by the same CU).
// Reference: gat2.py:234 (atom -> fragment sum), :296-326 (fragment graph), :436-440 (act(dropout)), :820-823 (readout).
//
// Padding molecules of a static-shape batch (index >= *counts_dev) are not molecule-contiguous (fn_stage_padded points their
// items round-robin at the reserved slots); their extents still partition the padding rows, so their workgroups write zeros:
// nothing of a real molecule reads them and the loss weighs them with 0 (their true gradients are 0 as well).

struct TailFwdArgs {
    const MolExt* ext;  int n_mols;  const int32_t* counts_dev;
    const float* atoms_new;  const int32_t* a2f_rowptr;  const int32_t* a2f_perm;  int32_t a2f_base, a2f_items;      // atom -> fragment CSR
    float* frags;                                                  // [F,128] fragment sums (kept for the backward pass)
    const float* att;  int att_w, dst_off, src_off, mid_off;       // f [H, 2d + 128]
    float *s_dst, *s_src;                                          // [F,H] node scalars (scratch)
    const float* feat;  float* s_sorted;                           // new_fbond rows -> the fragment graph's edge term [H][m]
    GatFwdArgs G;                                                  // the fragment graph's attention (mode-0 edge term = s_sorted)
    const float* y_atoms;  float* pooled;                          // readout [n_mols, 256] (nullable)
    int force_global;                                              // dev / test: every molecule takes the global-memory path
};

constexpr int kTailNF = 32, kTailME = 128;      // LDS path: fragments / fragment-graph edges of one molecule
// the backward's tile: 24 fragments keep its LDS at 45 KB = three workgroups per CU, i.e. all 528 molecules of a B = 512 step
// resident at once (at 32 fragments / 57 KB the last 16 started when the first ones finished); 8 heads need 64 partial rows
template <int H> constexpr int tail_bwd_nf() { return H == 8 ? 32 : 24; }

template <int H>
struct TailFwdLds {
    float F[kTailNF][FN_D];            // fragment sums
    float S[kRows][2 * FN_D];          // readout partials per half-wave: atoms | fragments
    float sd[kTailNF][H], ss[kTailNF][H];
    float e[H][kTailME];               // edge term at the molecule's destination-sorted positions
    int rp[kTailNF + 1];               // in-edge extents of the molecule's fragments, local positions
    int src[kTailME];                  // source fragment (local) at each position
};

// readout of the atoms' half: rows i = hw, hw + 8, ... of the molecule (block_rows_sum's order), four loads in flight
__device__ __forceinline__ float4 tail_rows_sum(const float* __restrict__ rows, int r0, int cnt, int hw, int lane) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i0 = hw; i0 < cnt; i0 += 4 * kRows) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kRows < cnt ? i0 + u * kRows : i0;
            v[u] = ld4_off(rows, (uint32_t)(r0 + i) * (FN_D * 4) + lane * 16);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * kRows < cnt) { acc.x += v[u].x;  acc.y += v[u].y;  acc.z += v[u].z;  acc.w += v[u].w; }
    }
    return acc;
}

template <int H>
__device__ __forceinline__ void tail_fwd_lds(const TailFwdArgs& T, const MolExt& x, int mol, TailFwdLds<H>& L) {
    constexpr int LPH = 32 / H;
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5, head = lane / LPH, j = lane % LPH;
    const fn_gat_plan& pl = T.G.pl;
    const int m = (int)pl.m, F = (int)pl.n;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // ---- round trip 1.  The two dependent chains start first (loads return in order: what is issued behind them does not
    // delay them): the fragment's atom extent and the connection id of half-wave hw's first fragment / first position; then
    // the molecule's slice of the plan (-> LDS), the atoms' half of the readout (depends on nothing here), the attention vector
    auto chain_heads = [&](int fl, i32x2u& rp, int& eid) {
        rp = ldp(T.a2f_rowptr + (x.f0 + fl < F ? x.f0 + fl : F - 1));
        eid = pl.eid_d[x.ec0 + fl < m ? x.ec0 + fl : m - 1];
    };
    i32x2u rp_n;
    int eid_n;
    chain_heads(hw, rp_n, eid_n);
    const int rpd_v = (int)threadIdx.x <= x.nf ? pl.rowptr_d[x.f0 + threadIdx.x] : 0;
    const int src_v = (int)threadIdx.x < x.mec ? pl.src_d[x.ec0 + threadIdx.x] : 0;
    const float4 accA = T.pooled ? tail_rows_sum(T.y_atoms, x.a0, x.na, hw, lane) : zero;
    const float4 ad = ld4(T.att + head * T.att_w + T.dst_off + j * 4);
    const float4 as = ld4(T.att + head * T.att_w + T.src_off + j * 4);
    float4 am[H];
#pragma unroll
    for (int q = 0; q < H; ++q) am[q] = ld4(T.att + q * T.att_w + T.mid_off + lane * 4);
    // ---- fragment sums (ascending atom order) + node scalars, and the edge term of the fragment graph: half-wave hw takes
    // fragment hw + 8k and position hw + 8k; the two chains' loads travel together
    const int iters = ((x.nf > x.mec ? x.nf : x.mec) + kRows - 1) / kRows;
    for (int k = 0; k < iters; ++k) {
        const int fl = hw + kRows * k;
        const bool hf = fl < x.nf, he = fl < x.mec;
        const i32x2u rp = rp_n;
        const int eid = eid_n;
        const int beg = rp.x - T.a2f_base, deg = hf ? rp.y - rp.x : 0;
        const bool real = he && eid < pl.m_real;
        int p0 = beg + (lane < deg ? lane : (deg > 0 ? deg - 1 : 0));
        p0 = p0 < T.a2f_items ? p0 : T.a2f_items - 1;               // (no fragment here: a valid entry, unused)
        const int mine0 = T.a2f_perm[p0];
        const float4 fv = ld4_off(T.feat, (uint32_t)(real ? eid : 0) * (FN_D * 4) + lane * 16);
        if (k + 1 < iters) chain_heads(fl + kRows, rp_n, eid_n);
        float4 acc = zero;
        for (int c0 = 0; c0 < deg; c0 += 32) {
            const int cn = deg - c0 < 32 ? deg - c0 : 32;
            const int mine = c0 == 0 ? mine0 : T.a2f_perm[beg + c0 + (lane < cn ? lane : cn - 1)];
            for (int i0 = 0; i0 < cn; i0 += 4) {               // four rows in flight
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int a = __shfl(mine, i0 + u < cn ? i0 + u : cn - 1, 32);
                    v[u] = ld4_off(T.atoms_new, (uint32_t)a * (FN_D * 4) + lane * 16);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u < cn) { acc.x += v[u].x;  acc.y += v[u].y;  acc.z += v[u].z;  acc.w += v[u].w; }
            }
        }
        if (hf) {
            st4(T.frags + (size_t)(x.f0 + fl) * FN_D + lane * 4, acc);        // the backward pass reads the sums
            st4(&L.F[fl][lane * 4], acc);
            const float pd = head_sum<LPH>(dot4(acc, ad)), ps = head_sum<LPH>(dot4(acc, as));
            if (j == 0) { L.sd[fl][head] = pd;  L.ss[fl][head] = ps; }
        }
        if (he) {
            float mine_e = 0.f;
#pragma unroll
            for (int q = 0; q < H; ++q) {
                const float dd = head_sum<32>(dot4(fv, am[q]));
                if (lane == q) mine_e = dd;
            }
            if (lane < H) L.e[lane][fl] = real ? mine_e : 0.f;
        }
    }
    if ((int)threadIdx.x <= x.nf) L.rp[threadIdx.x] = rpd_v - pl.pos_base_d - x.ec0;
    if ((int)threadIdx.x < x.mec) L.src[threadIdx.x] = src_v - x.f0;
    __syncthreads();

    // ---- fragment-graph attention out of LDS (gat2.py:296-326): every lane of a head walks the fragment's in-edges
    const fn_act_epilogue& ep = T.G.ep;
    const float slope = T.G.slope;
    const uint64_t rng_base = ep.offset + ((ep.p > 0.f && ep.offset_dev) ? *ep.offset_dev : 0);
    float4 accF = zero;
    for (int t = hw; t < x.nf; t += kRows) {
        const int beg = L.rp[t], end = L.rp[t + 1];
        const float sd = L.sd[t][head];
        float mx = -INFINITY;
        for (int k = beg; k < end; ++k) {
            const float z = L.e[head][k] + sd + L.ss[L.src[k]][head];
            mx = fmaxf(mx, fmaxf(z, slope * z));
        }
        float den = 0.f;
        for (int k = beg; k < end; ++k) {
            const float z = L.e[head][k] + sd + L.ss[L.src[k]][head];
            den += __expf(fmaxf(z, slope * z) - mx);
        }
        const float inv = __builtin_amdgcn_rcpf(den);
        float4 acc = zero;
        for (int k = beg; k < end; ++k) {
            const int sl = L.src[k];
            const float z = L.e[head][k] + sd + L.ss[sl][head];
            const float pk = __expf(fmaxf(z, slope * z) - mx) * inv;
            if ((k - beg) % LPH == j) T.G.p_sorted[(size_t)head * m + x.ec0 + k] = z > 0.f ? pk : -pk;      // sign = LeakyReLU branch
            fma4(acc, pk, *reinterpret_cast<const float4*>(&L.F[sl][lane * 4]));
        }
        float4 r = acc;                                        // act(dropout(.)): the Philox block index of k_dropout_act
        if (ep.p > 0.f) {
            const uint4 rnd = philox4x32(rng_base + (uint64_t)(x.f0 + t) * 32 + lane, ep.seed);
            const float ik = ep.p < 1.f ? 1.f / (1.f - ep.p) : 0.f;
            r.x *= keep_scale(rnd.x, ep.p, ik);  r.y *= keep_scale(rnd.y, ep.p, ik);
            r.z *= keep_scale(rnd.z, ep.p, ik);  r.w *= keep_scale(rnd.w, ep.p, ik);
        }
        if (ep.relu) { r.x = fmaxf(r.x, 0.f);  r.y = fmaxf(r.y, 0.f);  r.z = fmaxf(r.z, 0.f);  r.w = fmaxf(r.w, 0.f); }
        st4(ep.y + (size_t)(x.f0 + t) * FN_D + lane * 4, r);
        accF.x += r.x;  accF.y += r.y;  accF.z += r.z;  accF.w += r.w;
    }
    if (!T.pooled) return;
    // ---- readout: the eight half-waves' partial rows added in block_rows_sum's order
    st4(&L.S[hw][lane * 4], accA);
    st4(&L.S[hw][FN_D + lane * 4], accF);
    __syncthreads();
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRows; ++w) v += L.S[w][threadIdx.x];
    T.pooled[(size_t)mol * 2 * FN_D + threadIdx.x] = v;
}

// a molecule beyond the LDS tile: the stand-alone kernels' cores on the molecule's rows, through global memory
template <int H>
__device__ __forceinline__ void tail_fwd_global(const TailFwdArgs& T, const MolExt& x, int mol, float (*sS)[2 * FN_D]) {
    constexpr int LPH = 32 / H;
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5, head = lane / LPH, j = lane % LPH;
    const fn_gat_plan& pl = T.G.pl;
    const int m = (int)pl.m;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // ---- phase 1: fragment sums (ascending atom order = the reference's sequential scatter_add), node scalars, edge term
    {
        const float4 ad = ld4(T.att + head * T.att_w + T.dst_off + j * 4);
        const float4 as = ld4(T.att + head * T.att_w + T.src_off + j * 4);
        for (int f = x.f0 + hw; f < x.f0 + x.nf; f += kRows) {
            const i32x2u rp = ldp(T.a2f_rowptr + f);
            const int beg = rp.x - T.a2f_base, deg = rp.y - rp.x;
            float4 acc = zero;
            for (int c0 = 0; c0 < deg; c0 += 32) {
                const int cn = deg - c0 < 32 ? deg - c0 : 32;
                const int mine = T.a2f_perm[beg + c0 + (lane < cn ? lane : cn - 1)];
                for (int i0 = 0; i0 < cn; i0 += 4) {               // four rows in flight
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int a = __shfl(mine, i0 + u < cn ? i0 + u : cn - 1, 32);
                        v[u] = ld4_off(T.atoms_new, (uint32_t)a * (FN_D * 4) + lane * 16);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (i0 + u < cn) { acc.x += v[u].x;  acc.y += v[u].y;  acc.z += v[u].z;  acc.w += v[u].w; }
                }
            }
            st4(T.frags + (size_t)f * FN_D + lane * 4, acc);
            const float pd = head_sum<LPH>(dot4(acc, ad)), ps = head_sum<LPH>(dot4(acc, as));
            if (j == 0) { T.s_dst[(size_t)f * H + head] = pd;  T.s_src[(size_t)f * H + head] = ps; }
        }
        float4 a[H];
#pragma unroll
        for (int q = 0; q < H; ++q) a[q] = ld4(T.att + q * T.att_w + T.mid_off + lane * 4);
        for (int pos = x.ec0 + hw; pos < x.ec0 + x.mec; pos += kRows) {
            const int eid = pl.eid_d[pos];
            float mine = 0.f;
            if (eid < pl.m_real) {                                 // uniform inside the half-wave
                const float4 v = ld4(T.feat + (size_t)eid * FN_D + lane * 4);
#pragma unroll
                for (int q = 0; q < H; ++q) {
                    const float dd = head_sum<32>(dot4(v, a[q]));
                    if (lane == q) mine = dd;
                }
            }
            if (lane < H) T.s_sorted[(size_t)lane * m + pos] = mine;
        }
    }
    __syncthreads();            // workgroup-scope release/acquire: the rows and scalars above are read below by other waves

    // ---- phase 2: fragment-graph attention over the molecule's fragments, act(dropout(.)) epilogue -> y_frags
    gat_fwd_rows<H, 0>(T.G, nullptr, x.f0, x.f0 + x.nf, (x.nf + kRows - 1) / kRows);
    if (!T.pooled) return;
    __syncthreads();

    // ---- phase 3: readout, cat(sum of the molecule's y_atoms rows, sum of its y_frags rows) -- block_rows_sum's order
    st4(&sS[hw][lane * 4], tail_rows_sum(T.y_atoms, x.a0, x.na, hw, lane));
    st4(&sS[hw][FN_D + lane * 4], tail_rows_sum(T.G.ep.y, x.f0, x.nf, hw, lane));
    __syncthreads();
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kRows; ++w) v += sS[w][threadIdx.x];
    T.pooled[(size_t)mol * 2 * FN_D + threadIdx.x] = v;
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_tail_fwd(TailFwdArgs T) {
    __shared__ TailFwdLds<H> L;
    const int mol = (int)blockIdx.x, lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const MolExt x = T.ext[mol];
    const int n_real = T.counts_dev ? *T.counts_dev : T.n_mols;
    const int m = (int)T.G.pl.m;
    if (mol >= n_real) {                                           // padding molecule: zeros over its share of the padding rows
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int f = x.f0 + hw; f < x.f0 + x.nf; f += kRows) {
            st4(T.frags + (size_t)f * FN_D + lane * 4, zero);
            st4(T.G.ep.y + (size_t)f * FN_D + lane * 4, zero);
        }
        for (int i = threadIdx.x; i < x.mec * H; i += kBlock) T.G.p_sorted[(size_t)(i / x.mec) * m + x.ec0 + i % x.mec] = 0.f;
        if (T.pooled) T.pooled[(size_t)mol * 2 * FN_D + threadIdx.x] = 0.f;
        return;
    }
    if (x.nf <= kTailNF && x.mec <= kTailME && T.force_global == 0) tail_fwd_lds<H>(T, x, mol, L);
    else tail_fwd_global<H>(T, x, mol, L.S);
}

struct TailBwdArgs {
    const MolExt* ext;  int n_mols;  const int32_t* counts_dev;
    const float *g_atoms, *g_frags, *g_pooled;                     // dL/d(out_atoms), dL/d(out_frags), dL/d(readout): each nullable
    const float *y_atoms, *y_frags;  float scale;                  // saved outputs relu(dropout(.)): > 0 where kept and passed
    float *g_pre_atoms, *g_pre_frags;
    GatBwdDstArgs D;  GatBwdSrcArgs S;  RowDotsBwdArgs R;          // fragment graph: destination pass, source pass, edge-term backward
    const int64_t* a2f_index;  int64_t n_atoms;                    // atom -> fragment
    int force_global;                                              // dev / test: every molecule takes the global-memory path
    // one-pass backward of the atom level (gat_bwd_one.inc): the dots of the finished atom rows, c = <g, out>, u = <g, out2> - c sigma,
    // written where the rows are (cu_c == null: not wanted).  The fragment-bond rows' dots ride in R (RowDotsBwdArgs::cu_*).
    const float *cu_out, *cu_out2, *cu_sigma;
    float *cu_c, *cu_u;
};
// the two per-head dots of one finished gradient row held by a half-wave (lane: four columns), see gat_bwd_one.inc
// (sg: sigma[row, this lane's head], loaded by the caller together with the rows -- loaded here it would be one more dependent round trip)
template <int H>
__device__ __forceinline__ void row_cu_dots(float4 g, float4 o, float4 o2, float sg, float* c, float* u, int64_t row, int lane) {
    constexpr int LPH = 32 / H;
    const float cc = head_sum<LPH>(dot4(g, o));
    const float uu = head_sum<LPH>(dot4(g, o2));
    if (lane % LPH == 0) {
        const int64_t at = row * H + lane / LPH;
        c[at] = cc;
        if (u) u[at] = uu - cc * sg;       // (u == null: only c is wanted; o2 / sg are zeros then)
    }
}

template <int H>
struct TailBwdLds {
    static constexpr int kTailNF = tail_bwd_nf<H>();
    float FG[2 * kTailNF * FN_D];      // fragment sums h | dL/d(pre-activation fragment rows); afterwards the partial rows
    float GH[kTailNF][FN_D];           // dL/d(fragment sums)
    float p[H][kTailME], dz[H][kTailME];      // signed probabilities, dz (first the raw dots) at destination-sorted positions
    float dzo[kTailME][H];             // dz by local connection id (original edge order)
    float gsd[kTailNF][H];
    int rpd[kTailNF + 1], rps[kTailNF + 1], src[kTailME], eid[kTailME], dst_s[kTailME], dpos_s[kTailME];
};

template <int H>
__device__ __forceinline__ void tail_bwd_lds(const TailBwdArgs& T, const MolExt& x, int mol, TailBwdLds<H>& L) {
    constexpr int LPH = 32 / H;
    const int tid = threadIdx.x, lane = tid & 31, hw = tid >> 5, head = lane / LPH, j = lane % LPH;
    const fn_gat_plan& pl = T.D.pl;
    const int m = (int)pl.m;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float sc = T.scale, slope = T.D.slope;
    constexpr int kTailNF = tail_bwd_nf<H>();
    float* const Fr = L.FG;                          // [kTailNF][128]
    float* const Gr = L.FG + kTailNF * FN_D;         // [kTailNF][128]
    auto row4 = [&](const float* base, int r) { return *reinterpret_cast<const float4*>(base + r * FN_D + lane * 4); };
    // ---- round trip 1: the molecule's slice of the plan, its probabilities, rows and gates -> LDS
    const int es0 = x.c0 + (pl.m > pl.m_real ? x.f0 : 0);          // first by-source item of the molecule (cf. mol_extents_body)
    if (tid <= x.nf) {
        L.rpd[tid] = pl.rowptr_d[x.f0 + tid] - pl.pos_base_d - x.ec0;
        L.rps[tid] = pl.rowptr_s[x.f0 + tid] - pl.pos_base_s - es0;
    }
    if (tid < x.mec) {
        L.src[tid] = pl.src_d[x.ec0 + tid] - x.f0;
        L.eid[tid] = pl.eid_d[x.ec0 + tid];
        L.dst_s[tid] = pl.dst_s[es0 + tid] - x.f0;
        L.dpos_s[tid] = pl.dpos_s[es0 + tid] - x.ec0;
#pragma unroll
        for (int h = 0; h < H; ++h) L.p[h][tid] = T.D.p_sorted[(size_t)h * m + x.ec0 + tid];
    }
    const float4 gpA = T.g_pooled ? ld4(T.g_pooled + (size_t)mol * 2 * FN_D + lane * 4) : zero;
    const float4 gpF = T.g_pooled ? ld4(T.g_pooled + (size_t)mol * 2 * FN_D + FN_D + lane * 4) : zero;
    auto gate = [&](const float* g_rows, int64_t row, const float4& gp, const float4& v) {
        float4 g = gp;
        if (g_rows) { const float4 a = ld4(g_rows + (size_t)row * FN_D + lane * 4);  g.x += a.x;  g.y += a.y;  g.z += a.z;  g.w += a.w; }
        return make_float4(v.x > 0.f ? g.x * sc : 0.f, v.y > 0.f ? g.y * sc : 0.f, v.z > 0.f ? g.z * sc : 0.f, v.w > 0.f ? g.w * sc : 0.f);
    };
    for (int f = hw; f < x.nf; f += kRows) {
        const float4 hr = ld4(T.D.h + (size_t)(x.f0 + f) * FN_D + lane * 4);
        const float4 yv = ld4(T.y_frags + (size_t)(x.f0 + f) * FN_D + lane * 4);
        st4(Fr + f * FN_D + lane * 4, hr);
        st4(Gr + f * FN_D + lane * 4, gate(T.g_frags, x.f0 + f, gpF, yv));
    }
    const float4 ad = ld4(T.S.att + head * T.S.att_w + T.S.dst_off + j * 4);
    const float4 as = ld4(T.S.att + head * T.S.att_w + T.S.src_off + j * 4);
    float4 am[H];
#pragma unroll
    for (int q = 0; q < H; ++q) am[q] = ld4(T.R.A + q * T.R.lda + T.R.off + lane * 4);
    // the first batch of the last phase (the molecule's atoms: fragment id, saved output, incoming gradient) and the first
    // connection row of this half-wave (edge term's backward) depend on nothing computed here: in flight during the passes
    int fr0[4];
    float4 yv0[4], ga0[4], ov0[4], o2v0[4];
    float sg0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = x.a0 + (hw + u * kRows < x.na ? hw + u * kRows : 0);
        const int ic = i < (int)T.n_atoms ? i : (int)T.n_atoms - 1;
        fr0[u] = (int)T.a2f_index[ic] - x.f0;
        yv0[u] = ld4(T.y_atoms + (size_t)ic * FN_D + lane * 4);
        ga0[u] = T.g_atoms ? ld4(T.g_atoms + (size_t)ic * FN_D + lane * 4) : zero;
        ov0[u] = T.cu_c ? ld4(T.cu_out + (size_t)ic * FN_D + lane * 4) : zero;       // (one-pass dots of the atom rows, below)
        o2v0[u] = T.cu_out2 ? ld4(T.cu_out2 + (size_t)ic * FN_D + lane * 4) : zero;
        sg0[u] = T.cu_out2 ? T.cu_sigma[(size_t)ic * H + lane / (32 / H)] : 0.f;
    }
    const int el0 = hw < x.nc ? hw : 0;
    const float4 fv0 = x.nc > 0 ? ld4(T.R.feat + (size_t)(x.c0 + el0) * FN_D + lane * 4) : zero;
    const float4 av0 = (x.nc > 0 && T.R.addend) ? ld4(T.R.addend + (size_t)(x.c0 + el0) * FN_D + lane * 4) : zero;
    const float4 cv0 = (x.nc > 0 && T.R.cu_out2) ? ld4(T.R.cu_out2 + (size_t)(x.c0 + el0) * FN_D + lane * 4) : zero;
    const float cs0 = (x.nc > 0 && T.R.cu_out2) ? T.R.cu_sigma[(size_t)(x.c0 + el0) * H + lane / (32 / H)] : 0.f;
    __syncthreads();

    // ---- destination pass: dp_e = <g[t], h[src_e]>, c = sum p dp, dz_e = p (dp - c) LeakyReLU'
    for (int t = hw; t < x.nf; t += kRows) {
        const float4 g = row4(Gr, t);
        const int beg = L.rpd[t], end = L.rpd[t + 1];
        float c = 0.f;
        for (int k = beg; k < end; ++k) {
            const float dp = head_sum<LPH>(dot4(g, row4(Fr, L.src[k])));
            if (j == 0) L.dz[head][k] = dp;
            c = fmaf(fabsf(L.p[head][k]), dp, c);
        }
        float gs = 0.f;
        for (int k = beg; k < end; ++k) {
            const float ps = L.p[head][k];
            const float dz = fabsf(ps) * (L.dz[head][k] - c) * ((__float_as_uint(ps) >> 31) ? slope : 1.f);
            gs += dz;
            if (j == 0) {
                L.dz[head][k] = dz;
                const int eid = L.eid[k];
                if (eid < pl.m_real) L.dzo[eid - x.c0][head] = dz;
            }
        }
        if (j == 0) L.gsd[t][head] = gs;
    }
    __syncthreads();

    // ---- source pass: g_h[s] = sum over out-edges p g[dst] + g_s_dst a_dst + (sum dz) a_src; partials of dL/da_dst, dL/da_src
    float4 qd = zero, qs = zero;
    for (int s = hw; s < x.nf; s += kRows) {
        float4 acc = zero;
        float gss = 0.f;
        for (int i = L.rps[s]; i < L.rps[s + 1]; ++i) {
            const int pos = L.dpos_s[i];
            fma4(acc, fabsf(L.p[head][pos]), row4(Gr, L.dst_s[i]));
            gss += L.dz[head][pos];
        }
        const float gsd = L.gsd[s][head];
        fma4(acc, gsd, ad);
        fma4(acc, gss, as);
        st4(&L.GH[s][lane * 4], acc);
        const float4 hr = row4(Fr, s);
        fma4(qd, gsd, hr);
        fma4(qs, gss, hr);
    }
    // ---- the edge term's backward over the molecule's connections: dL/d(new_fbond) rows, partials of f's middle block
    float4 q[H];
#pragma unroll
    for (int h = 0; h < H; ++h) q[h] = zero;
    for (int el = hw; el < x.nc; el += kRows) {
        const float4 v = el == hw ? fv0 : ld4(T.R.feat + (size_t)(x.c0 + el) * FN_D + lane * 4);
        float4 acc = !T.R.addend ? zero : (el == hw ? av0 : ld4(T.R.addend + (size_t)(x.c0 + el) * FN_D + lane * 4));
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const float dz = L.dzo[el][h];
            fma4(acc, dz, am[h]);
            fma4(q[h], dz, v);
        }
        st4(T.R.g_feat + (size_t)(x.c0 + el) * FN_D + lane * 4, acc);
        if (T.R.cu_c)           // the raw row of the fragment-bond level IS this edge term's feature row
            row_cu_dots<H>(acc, v, (el == hw || !T.R.cu_out2) ? cv0 : ld4(T.R.cu_out2 + (size_t)(x.c0 + el) * FN_D + lane * 4),
                           (el == hw || !T.R.cu_out2) ? cs0 : T.R.cu_sigma[(size_t)(x.c0 + el) * H + lane / (32 / H)], T.R.cu_c, T.R.cu_u, x.c0 + el, lane);
    }
    __syncthreads();            // every read of the h / g rows is done: their space takes the partial rows
    float* const P = L.FG;
    st4(P + hw * 2 * FN_D + lane * 4, qd);
    st4(P + hw * 2 * FN_D + FN_D + lane * 4, qs);
    __syncthreads();
    {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kRows; ++w) v += P[w * 2 * FN_D + tid];
        T.S.part_a[part_at(T.S.part_ld, mol, tid)] = v;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < H; ++h) st4(P + (hw * H + h) * FN_D + lane * 4, q[h]);
    __syncthreads();
    for (int c = tid; c < H * FN_D; c += kBlock) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kRows; ++w) v += P[w * H * FN_D + c];
        T.R.part[part_at(T.R.part_ld, mol, c)] = v;
    }
    // ---- dL/d(atoms_new) = gate(dL/d(out_atoms) + the readout's share) + dL/d(fragment sums)[fragment of the atom]
    for (int i0 = hw; i0 < x.na; i0 += 4 * kRows) {
        int fr[4];
        float4 yv[4], ga[4], ov[4], o2v[4];
        float sg[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 == hw) { fr[u] = fr0[u];  yv[u] = yv0[u];  ga[u] = ga0[u];  ov[u] = ov0[u];  o2v[u] = o2v0[u];  sg[u] = sg0[u];  continue; }
            if (T.cu_c) {
                const size_t ia = (size_t)(x.a0 + (i0 + u * kRows < x.na ? i0 + u * kRows : i0));
                ov[u] = ld4(T.cu_out + ia * FN_D + lane * 4);  o2v[u] = T.cu_out2 ? ld4(T.cu_out2 + ia * FN_D + lane * 4) : zero;
                sg[u] = T.cu_out2 ? T.cu_sigma[ia * H + lane / (32 / H)] : 0.f;
            } else { ov[u] = zero;  o2v[u] = zero;  sg[u] = 0.f; }
            const int i = x.a0 + (i0 + u * kRows < x.na ? i0 + u * kRows : i0);
            fr[u] = (int)T.a2f_index[i] - x.f0;
            yv[u] = ld4(T.y_atoms + (size_t)i * FN_D + lane * 4);
            ga[u] = T.g_atoms ? ld4(T.g_atoms + (size_t)i * FN_D + lane * 4) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i0 + u * kRows >= x.na) continue;
            const float4 g = make_float4(ga[u].x + gpA.x, ga[u].y + gpA.y, ga[u].z + gpA.z, ga[u].w + gpA.w);
            const float4 a = make_float4(yv[u].x > 0.f ? g.x * sc : 0.f, yv[u].y > 0.f ? g.y * sc : 0.f, yv[u].z > 0.f ? g.z * sc : 0.f,
                                         yv[u].w > 0.f ? g.w * sc : 0.f);
            float4 v = *reinterpret_cast<const float4*>(&L.GH[fr[u]][lane * 4]);
            v.x += a.x;  v.y += a.y;  v.z += a.z;  v.w += a.w;
            st4(T.g_pre_atoms + (size_t)(x.a0 + i0 + u * kRows) * FN_D + lane * 4, v);
            if (T.cu_c) row_cu_dots<H>(v, ov[u], o2v[u], sg[u], T.cu_c, T.cu_u, x.a0 + i0 + u * kRows, lane);
        }
    }
}

// a molecule beyond the LDS tile: the stand-alone kernels' cores on the molecule's rows, through global memory
template <int H>
__device__ __forceinline__ void tail_bwd_global(const TailBwdArgs& T, const MolExt& x, int mol, float (*sA)[2 * FN_D]) {
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float sc = T.scale;
    auto gate = [&](const float* g_rows, int64_t row, int pool_off, const float* y_rows) {
        float4 g = g_rows ? ld4(g_rows + (size_t)row * FN_D + lane * 4) : zero;
        if (T.g_pooled) {
            const float4 gp = ld4(T.g_pooled + (size_t)mol * 2 * FN_D + pool_off + lane * 4);
            if (g_rows) { g.x += gp.x;  g.y += gp.y;  g.z += gp.z;  g.w += gp.w; } else g = gp;
        }
        const float4 v = ld4(y_rows + (size_t)row * FN_D + lane * 4);
        return make_float4(v.x > 0.f ? g.x * sc : 0.f, v.y > 0.f ? g.y * sc : 0.f, v.z > 0.f ? g.z * sc : 0.f, v.w > 0.f ? g.w * sc : 0.f);
    };

    // ---- phase 1: dL/d(pre-activation fragment rows) = gate(dL/d(out_frags) + the readout's share)
    for (int f = x.f0 + hw; f < x.f0 + x.nf; f += kRows) st4(T.g_pre_frags + (size_t)f * FN_D + lane * 4, gate(T.g_frags, f, FN_D, T.y_frags));
    __syncthreads();
    // ---- phase 2: fragment graph, destination pass
    const int rph = (x.nf + kRows - 1) / kRows;
    gat_bwd_dst_rows<H, 0, kBwdRows>(T.D, nullptr, x.f0, x.f0 + x.nf, rph, mol);
    __syncthreads();
    // ---- phase 3: source pass (-> dL/d(fragment sums), attention-vector partials) and the edge term's backward over the
    // molecule's fragment connections (-> dL/d(new_fbond) rows, partials of f's middle block)
    gat_bwd_src_rows<H, kBwdRows>(T.S, sA, x.f0, x.f0 + x.nf, rph, mol);
    __syncthreads();
    row_dots_sorted_bwd_range(T.R, reinterpret_cast<float(*)[FN_D]>(&sA[0][0]), x.c0, x.c0 + x.nc, mol);
    // ---- phase 4: dL/d(atoms_new) = gate(dL/d(out_atoms) + the readout's share) + dL/d(fragment sums)[fragment of the atom]
    // (the trailing barrier of the edge-term body orders the g_h rows of phase 3 before these reads)
    for (int i = x.a0 + hw; i < x.a0 + x.na; i += kRows) {
        const int64_t fr = T.a2f_index[i];
        float4 v = ld4(T.S.g_h + (size_t)fr * FN_D + lane * 4);
        const float4 a = gate(T.g_atoms, i, 0, T.y_atoms);
        v.x += a.x;  v.y += a.y;  v.z += a.z;  v.w += a.w;
        st4(T.g_pre_atoms + (size_t)i * FN_D + lane * 4, v);
        if (T.cu_c)
            row_cu_dots<H>(v, ld4(T.cu_out + (size_t)i * FN_D + lane * 4),
                           T.cu_out2 ? ld4(T.cu_out2 + (size_t)i * FN_D + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f),
                           T.cu_out2 ? T.cu_sigma[(size_t)i * H + lane / (32 / H)] : 0.f, T.cu_c, T.cu_u, i, lane);
    }
}

template <int H>
__global__ __launch_bounds__(kBlock) void k_tail_bwd(TailBwdArgs T, AdamRide R) {
    static_assert(kBwdRows == kRows && kBwdRows * 32 == kBlock, "the cores run 8 half-waves per block");
    constexpr int kTailNF = tail_bwd_nf<H>();
    static_assert(sizeof(TailBwdLds<H>) <= 64 * 1024 && 2 * kTailNF >= kRows * H && 2 * kTailNF * FN_D >= kRows * 2 * FN_D, "LDS tile");
    __shared__ TailBwdLds<H> L;
    if (R.nblk && (int)blockIdx.x >= R.first) { adam_ride(R);  return; }      // FN_TUNE_RIDER_AT = 1: the head's Adam slice beside the molecules
    const int mol = (int)blockIdx.x, lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    const MolExt x = T.ext[mol];
    const int n_real = T.counts_dev ? *T.counts_dev : T.n_mols;
    if (mol >= n_real) {                                           // padding molecule: its rows' gradients are exactly 0
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = x.a0 + hw; i < x.a0 + x.na; i += kRows) st4(T.g_pre_atoms + (size_t)i * FN_D + lane * 4, zero);
        if (T.R.g_feat && !T.R.addend)
            for (int c = x.c0 + hw; c < x.c0 + x.nc; c += kRows) st4(T.R.g_feat + (size_t)c * FN_D + lane * 4, zero);
        // (zero gradient rows have zero dots)
        if (T.cu_c) for (int i = x.a0 * H + (int)threadIdx.x; i < (x.a0 + x.na) * H; i += kBlock) { T.cu_c[i] = 0.f;  if (T.cu_u) T.cu_u[i] = 0.f; }
        if (T.R.cu_c) for (int c = x.c0 * H + (int)threadIdx.x; c < (x.c0 + x.nc) * H; c += kBlock) { T.R.cu_c[c] = 0.f;  if (T.R.cu_u) T.R.cu_u[c] = 0.f; }
        T.S.part_a[part_at(T.S.part_ld, mol, (int)threadIdx.x)] = 0.f;                   // 2 * FN_D == kBlock columns
        for (int c = threadIdx.x; c < H * FN_D; c += kBlock) T.R.part[part_at(T.R.part_ld, mol, c)] = 0.f;
        return;
    }
    if (x.nf <= kTailNF && x.mec <= kTailME && x.nc <= kTailME && T.force_global == 0) tail_bwd_lds<H>(T, x, mol, L);
    else tail_bwd_global<H>(T, x, mol, reinterpret_cast<float(*)[2 * FN_D]>(L.FG));
}

