// shared_bodies.inc -- device bodies that a kernel of the operator surface (fragnet_hip.hip) and a combined launch of the engine
// (encoder.hip) both run, each defined once: the dropout + ReLU epilogue (k_dropout_act | k_enc_prologue) and the Adam update with its
// rider (k_adam | k_reduce_tasks, k_tail_bwd).  Included inside the anonymous namespace of both units.  No __global__ function may live
// here: one that is no template would be compiled into both.
// Likewise the pooling row sum (k_segment_sum128_wide, k_pool_cat, k_pool_cat_groups | k_frag_tail) and the destination-sorted edge
// term (k_row_dots_sorted | k_frag_tail): the order of additions that the read-outs' bit-for-bit statements rest on is written here, once.
// The pair heads' shared orders (v = W1^T w2, the last workgroup's dW2 / db2 / loss sums) are pair_bodies.inc's, under the same rule.

// The block row sum.  A 256-thread block adds the `deg` rows src[perm[beg + i] * ld + 0..127]: half-wave hw takes the items hw, hw + 8, ..
// in ascending order into one float4 per lane, from +0.0; the eight partial rows go to sS; after ONE barrier thread c < FN_D adds column
// c of them as ((0 + p0) + p1) + .. + p7 and hands the sum to fin(v); the other threads do not call fin.  A row with keep(row) == false
// enters as 0.0 and is not loaded.  A caller that loops over segments puts a barrier of its own behind the call, before sS is written
// again.  tests/pool_sum_ref.py restates this order in numpy.
template <class Keep, class Fin>
__device__ __forceinline__ void block_rows_sum(float (*sS)[FN_D], const float* __restrict__ src, int64_t ld,
                                                const int32_t* __restrict__ perm, int beg, int deg, Keep keep, Fin fin) {
    const int lane = threadIdx.x & 31, hw = threadIdx.x >> 5;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = hw; i < deg; i += kRows) {
        const int32_t row = perm[beg + i];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (keep(row)) v = ld4(src + (size_t)row * ld + lane * 4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    st4(&sS[hw][lane * 4], acc);
    __syncthreads();
    if (threadIdx.x < FN_D) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < kRows; ++w) v += sS[w][threadIdx.x];
        fin(v);
    }
}
struct KeepAllRows {          // the predicate of a plain sum
    __device__ __forceinline__ bool operator()(int32_t) const { return true; }
};

// The destination-sorted full-width edge term: s_sorted[q, pos] = <feat[eid(pos), :], A[q, off:off+128]> for q < J, 0 at loop positions
// (eid >= m_real); head-major [J][m].  One half-wave per position, dot4 per lane and the head_sum<32> butterfly; (vb, nb): this block's
// index / the number of blocks working on the level -- block_groups() for a virtual block.  NQ: the register rows, J <= NQ; where the
// caller's J is the constant NQ the q < J guards fold away.
template <int NQ>
__device__ __forceinline__ void row_dots_sorted_body(const float* __restrict__ feat, const float* __restrict__ A, int lda, int off, int J,
                                                     const fn_gat_plan& pl, float* __restrict__ s_sorted, int vb, int nb) {
    const int lane = threadIdx.x & 31;
    float4 a[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) a[q] = (q < J) ? ld4(A + q * lda + off + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t groups = (pl.m + kRows - 1) / kRows, per = (groups + nb - 1) / nb;
    const int64_t g0 = (int64_t)xcd_block(vb, nb) * per, g1 = g0 + per < groups ? g0 + per : groups;
    for (int64_t gi = g0; gi < g1; ++gi) {
        const int64_t pos = gi * kRows + (threadIdx.x >> 5);
        if (pos >= pl.m) continue;
        const int eid = pl.eid_d[pos];
        float mine = 0.f;
        if (eid < pl.m_real) {                       // uniform inside the half-wave
            const float4 v = ld4(feat + (size_t)eid * FN_D + lane * 4);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q < J) {
                    const float d = head_sum<32>(dot4(v, a[q]));
                    if (lane == q) mine = d;
                }
            }
        }
        if (lane < J) s_sorted[(size_t)lane * pl.m + pos] = mine;        // head-major [J][m]
    }
}

template <bool BWD>
__device__ __forceinline__ void dropout_act_body(const float* __restrict__ a, const float* __restrict__ y_saved, float* __restrict__ o,
                                                 int64_t numel, float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                                                 int relu, int vb, int nb, const uint8_t* __restrict__ gate = nullptr, int gate_w = 1) {
    // gate (the engine's prologue only: fn_encoder_forward_keep): one byte per row of gate_w elements, zero = the row reads as zero
    // BEFORE the mask is applied; the Philox words are those of the ungated tensor
    const int64_t n4 = (numel + 3) / 4;
    if (offset_dev) offset += *offset_dev;
    const float inv_keep = p < 1.f ? 1.f / (1.f - p) : 0.f;
    for (int64_t i = (int64_t)vb * blockDim.x + threadIdx.x; i < n4; i += (int64_t)nb * blockDim.x) {
        float m[4] = {1.f, 1.f, 1.f, 1.f};
        if (p > 0.f) {
            const uint4 r = philox4x32(offset + (uint64_t)i, seed);
            m[0] = keep_scale(r.x, p, inv_keep); m[1] = keep_scale(r.y, p, inv_keep);
            m[2] = keep_scale(r.z, p, inv_keep); m[3] = keep_scale(r.w, p, inv_keep);
        }
        const int64_t e0 = i * 4;
        if (e0 + 3 < numel) {
            float4 v = ld4(a + e0);
            if (gate) {      // one division per four elements: the row of e0, then walk (a row of fewer than four elements is walked past)
                int64_t row = e0 / gate_w;
                int rem = (int)(e0 - row * gate_w);
                float* V = &v.x;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!gate[row]) V[q] = 0.f;
                    if (++rem == gate_w) { rem = 0;  ++row; }
                }
            }
            float4 res;
            if (!BWD) {
                res = make_float4(v.x * m[0], v.y * m[1], v.z * m[2], v.w * m[3]);
                if (relu) { res.x = fmaxf(res.x, 0.f); res.y = fmaxf(res.y, 0.f); res.z = fmaxf(res.z, 0.f); res.w = fmaxf(res.w, 0.f); }
            } else {
                const float4 ys = relu ? ld4(y_saved + e0) : make_float4(1.f, 1.f, 1.f, 1.f);
                res = make_float4(ys.x > 0.f || !relu ? v.x * m[0] : 0.f, ys.y > 0.f || !relu ? v.y * m[1] : 0.f,
                                  ys.z > 0.f || !relu ? v.z * m[2] : 0.f, ys.w > 0.f || !relu ? v.w * m[3] : 0.f);
            }
            st4(o + e0, res);
        } else {
            for (int q = 0; q < 4 && e0 + q < numel; ++q) {
                float v = (gate && !gate[(e0 + q) / gate_w] ? 0.f : a[e0 + q]) * m[q];
                if (!BWD) { if (relu) v = fmaxf(v, 0.f); }
                else if (relu && !(y_saved[e0 + q] > 0.f)) v = 0.f;
                o[e0 + q] = v;
            }
        }
    }
}

// m' = beta1 m + (1 - beta1) g the way torch's lerp takes it: from the end whose weight is the larger one.  m + (g - m) * (1 - beta1) alone
// loses g where |g| < 2^-24 |m| (g - m rounds to -m): harmless while beta1 m dominates m' anyway, but at beta1 = 0, where m' is g, the
// parameter stood still.  (The branch is uniform; beta1 > 0.5, the default included, keeps the form and the bits it always had.)
__device__ __forceinline__ float adam_lerp(float m, float g, float beta1) {
    const float w = 1.f - beta1;
    return w < 0.5f ? m + (g - m) * w : g - (g - m) * beta1;
}
// torch.optim.Adam's update rule (no amsgrad) on one flat tensor: the reference's optimiser, finetune_gat2.py:257
// (vb, nb): this block's index / the number of blocks working on the tensor -- k_adam's own grid, or the riders' range of the
// deferred-reduction launch (AdamRide below)
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          int64_t n, float lr_over_bc1, float beta1, float beta2, float eps, float inv_sqrt_bc2, float wd,
                                          const int64_t* __restrict__ step_dev, const float* __restrict__ lr_dev, int vb, int nb) {
    if (step_dev) {      // captured in a hipGraph: step count and learning rate live in device memory, bias corrections here
        __shared__ float s2[2];
        if (threadIdx.x == 0) {
            const double st = (double)*step_dev;
            const double bc1 = 1.0 - pow((double)beta1, st), bc2 = 1.0 - pow((double)beta2, st);
            s2[0] = (float)((double)*lr_dev / bc1);
            s2[1] = (float)(1.0 / sqrt(bc2));
        }
        __syncthreads();
        lr_over_bc1 = s2[0];
        inv_sqrt_bc2 = s2[1];
    }
    const int64_t n4 = n / 4;
    for (int64_t i = (int64_t)vb * blockDim.x + threadIdx.x; i < n4; i += (int64_t)nb * blockDim.x) {
        float4 pp = ld4(p + i * 4), gg = ld4(g + i * 4), mm = ld4(m + i * 4), vv = ld4(v + i * 4);
        float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gq = G[q] + wd * P[q];
            M[q] = adam_lerp(M[q], gq, beta1);
            V[q] = V[q] * beta2 + (1.f - beta2) * gq * gq;
            P[q] -= lr_over_bc1 * (M[q] / (sqrtf(V[q]) * inv_sqrt_bc2 + eps));
        }
        st4(p + i * 4, pp); st4(m + i * 4, mm); st4(v + i * 4, vv);
    }
    if (vb == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = n4 * 4 + threadIdx.x;
        const float gq = g[i] + wd * p[i];
        const float mq = adam_lerp(m[i], gq, beta1);
        const float vq = v[i] * beta2 + (1.f - beta2) * gq * gq;
        m[i] = mq; v[i] = vq;
        p[i] -= lr_over_bc1 * (mq / (sqrtf(vq) * inv_sqrt_bc2 + eps));
    }
}
// An Adam update of parameters whose gradients were final BEFORE the encoder's backward pass began (the prediction head's, 84 % of a
// FragNetFineTune) rides in one of that pass's launches: blocks [first, first + nblk).  Independent of everything the pass computes;
// the step's own Adam launch then covers the rest of the flat buffer only (fn_encoder.adam_rider).  Where: FN_TUNE_RIDER_AT.
struct AdamRide {
    fn_adam_slice a;
    int first, nblk;             // nblk == 0: none
};
__device__ __forceinline__ void adam_ride(const AdamRide& R) {
    adam_body(R.a.p, R.a.g, R.a.m, R.a.v, R.a.n, 0.f, R.a.beta1, R.a.beta2, R.a.eps, 0.f, R.a.weight_decay, R.a.step_dev, R.a.lr_dev,
              (int)blockIdx.x - R.first, R.nblk);
}
inline AdamRide make_adam_ride(const fn_adam_slice* a, int first, int threads, int pieces) {
    AdamRide R{};
    if (a && a->n > 0) {
        const int64_t per = pieces > 0 ? pieces : 1;
        const int64_t nb = (a->n / 4 + per * threads - 1) / (per * threads);          // 16-byte pieces per thread
        R.a = *a;  R.first = first;  R.nblk = (int)(nb < 1 ? 1 : nb > 4096 ? 4096 : nb);
    }
    return R;
}
