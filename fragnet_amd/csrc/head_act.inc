// The activations of the prediction heads other than the ReLU fast path (include/fragnet_hip.h, fn_head_act), as epilogues of
// the dense-head products (dense_head.inc) and of the last Linear's kernels (k_small_linear_bwd, k_small_linear_loss).  Included
// into the anonymous namespace of head.hip.
//
// Reference: gat2.py:693-705 builds the head's activation from the finetune `act` key; torch's modules define f and f':
//   silu   u sigma(u)                              sigma(u) (1 + u (1 - sigma(u)))
//   gelu   u Phi(u)  (approximate = "none")          Phi(u) + u phi(u)
//   celu   max(0,u) + min(0, exp(u) - 1)  (alpha 1)  u > 0 ? 1 : exp(u)
//   selu   lambda (u > 0 ? u : alpha (exp(u) - 1))   u > 0 ? lambda : lambda alpha exp(u)
//   relu6  min(max(u, 0), 6)                         0 < u < 6
//   leakyrelu (0.01), prelu (one slope a)            u > 0 ? 1 : slope
// The forward saves u (the activation's argument: dropout(z) or z, by order) because neither silu nor gelu can be inverted from
// their output; the backward replays the dropout mask from the layer's Philox (seed, offset) -- never from a zero -- so that
//   d loss / d z = keep * f'(u) * d loss / d y
// holds in both orders (keep = mask / (1 - p)).  The PReLU slope's gradient is a partial sum per workgroup, combined once per head
// in a fixed order (k_head_act_param_grad).
constexpr float kSeluAlpha = 1.6732632423543772848170429916717f, kSeluScale = 1.0507009873554804934193349852946f;

template <int KIND> __device__ __forceinline__ float hact_f(float u, float a) {
    if constexpr (KIND == FN_ACT_RELU) return fmaxf(u, 0.f);
    else if constexpr (KIND == FN_ACT_SILU) return u / (1.f + expf(-u));
    else if constexpr (KIND == FN_ACT_GELU) return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
    else if constexpr (KIND == FN_ACT_CELU) return fmaxf(u, 0.f) + fminf(0.f, expm1f(u));
    else if constexpr (KIND == FN_ACT_SELU) return kSeluScale * (u > 0.f ? u : kSeluAlpha * expm1f(u));
    else if constexpr (KIND == FN_ACT_RELU6) return fminf(fmaxf(u, 0.f), 6.f);
    else if constexpr (KIND == FN_ACT_LEAKYRELU) return u > 0.f ? u : 0.01f * u;
    else return u > 0.f ? u : a * u;                                   // FN_ACT_PRELU
}
template <int KIND> __device__ __forceinline__ float hact_df(float u, float a) {
    if constexpr (KIND == FN_ACT_RELU) return u > 0.f ? 1.f : 0.f;
    else if constexpr (KIND == FN_ACT_SILU) { const float s = 1.f / (1.f + expf(-u));  return s * (1.f + u * (1.f - s)); }
    else if constexpr (KIND == FN_ACT_GELU) return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * 0.39894228040143268f * expf(-0.5f * u * u);
    else if constexpr (KIND == FN_ACT_CELU) return u > 0.f ? 1.f : expf(u);
    else if constexpr (KIND == FN_ACT_SELU) return u > 0.f ? kSeluScale : kSeluScale * kSeluAlpha * expf(u);
    else if constexpr (KIND == FN_ACT_RELU6) return u > 0.f && u < 6.f ? 1.f : 0.f;
    else if constexpr (KIND == FN_ACT_LEAKYRELU) return u > 0.f ? 1.f : 0.01f;
    else return u > 0.f ? 1.f : a;                                     // FN_ACT_PRELU
}

// what every thread of a launch needs once: the Philox counter base, 1 / (1 - p), the PReLU slope
struct HactRun { float p, ik, a; uint64_t ctr; };
__device__ __forceinline__ HactRun hact_run(const fn_head_act& h, int kind) {
    HactRun r;
    r.p = h.p;
    r.ik = h.p < 1.f ? 1.f / (1.f - h.p) : 0.f;
    r.ctr = h.p > 0.f ? h.offset + (h.offset_dev ? *h.offset_dev : 0) : 0;
    r.a = kind == FN_ACT_PRELU ? *h.prelu_w : 0.f;
    return r;
}
// keep / (1 - p) of the four elements e .. e+3 (e % 4 == 0) of the layer's output: the Philox block of k_dropout_act
__device__ __forceinline__ float4 hact_keep4(const fn_head_act& h, const HactRun& r, uint64_t e) {
    if (!(r.p > 0.f)) return make_float4(1.f, 1.f, 1.f, 1.f);
    const uint4 rnd = philox4x32(r.ctr + e / 4, h.seed);
    return make_float4(keep_scale(rnd.x, r.p, r.ik), keep_scale(rnd.y, r.p, r.ik), keep_scale(rnd.z, r.p, r.ik), keep_scale(rnd.w, r.p, r.ik));
}
// forward: z (bias added) -> y; u -> *pre
template <int KIND> __device__ __forceinline__ float4 hact_fwd4(const fn_head_act& h, const HactRun& r, float4 z, uint64_t e, float4& pre) {
    const float4 k = hact_keep4(h, r, e);
    if (h.order == FN_ACT_DROP_THEN_ACT) {
        pre = make_float4(z.x * k.x, z.y * k.y, z.z * k.z, z.w * k.w);
        return make_float4(hact_f<KIND>(pre.x, r.a), hact_f<KIND>(pre.y, r.a), hact_f<KIND>(pre.z, r.a), hact_f<KIND>(pre.w, r.a));
    }
    pre = z;
    return make_float4(hact_f<KIND>(z.x, r.a) * k.x, hact_f<KIND>(z.y, r.a) * k.y, hact_f<KIND>(z.z, r.a) * k.z, hact_f<KIND>(z.w, r.a) * k.w);
}
// backward: g = d loss / d y, u the saved argument -> d loss / d z;  dslope += the PReLU terms
template <int KIND> __device__ __forceinline__ float hact_bwd1(float g, float u, float k, bool act_then_drop, float a, float& dslope) {
    const float gf = act_then_drop ? g * k : g;                        // d loss / d f(u)
    if constexpr (KIND == FN_ACT_PRELU) dslope += u > 0.f ? 0.f : u * gf;
    const float gu = gf * hact_df<KIND>(u, a);                         // d loss / d u
    return act_then_drop ? gu : gu * k;
}
template <int KIND> __device__ __forceinline__ float4 hact_bwd4(const fn_head_act& h, const HactRun& r, float4 g, float4 u, uint64_t e, float& dslope) {
    const float4 k = hact_keep4(h, r, e);
    const bool ad = h.order == FN_ACT_ACT_THEN_DROP;
    return make_float4(hact_bwd1<KIND>(g.x, u.x, k.x, ad, r.a, dslope), hact_bwd1<KIND>(g.y, u.y, k.y, ad, r.a, dslope),
                       hact_bwd1<KIND>(g.z, u.z, k.z, ad, r.a, dslope), hact_bwd1<KIND>(g.w, u.w, k.w, ad, r.a, dslope));
}
// the kernels of the last Linear take the kind at run time (one uniform branch per row piece; they are not product-bound)
__device__ __forceinline__ float4 hact_bwd4_rt(const fn_head_act& h, const HactRun& r, float4 g, float4 u, uint64_t e, float& dslope) {
    switch (h.kind) {
        case FN_ACT_RELU: return hact_bwd4<FN_ACT_RELU>(h, r, g, u, e, dslope);
        case FN_ACT_SILU: return hact_bwd4<FN_ACT_SILU>(h, r, g, u, e, dslope);
        case FN_ACT_GELU: return hact_bwd4<FN_ACT_GELU>(h, r, g, u, e, dslope);
        case FN_ACT_CELU: return hact_bwd4<FN_ACT_CELU>(h, r, g, u, e, dslope);
        case FN_ACT_SELU: return hact_bwd4<FN_ACT_SELU>(h, r, g, u, e, dslope);
        case FN_ACT_RELU6: return hact_bwd4<FN_ACT_RELU6>(h, r, g, u, e, dslope);
        case FN_ACT_LEAKYRELU: return hact_bwd4<FN_ACT_LEAKYRELU>(h, r, g, u, e, dslope);
        default: return hact_bwd4<FN_ACT_PRELU>(h, r, g, u, e, dslope);
    }
}
// one partial of the PReLU slope's gradient per workgroup: lanes, then waves in order (every thread of the block calls it;
// s: WAVES floats of LDS that nobody reads any more -- the dense kernels pass their dynamic LDS, which then stays at 64 KB)
template <int WAVES, typename LdsPtr> __device__ __forceinline__ void hact_block_partial(float v, float* part, int slot, LdsPtr s) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = s[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) t += s[w];
        part[slot] = t;
    }
}
// d loss / d slope = the sum of all partials of a head, in index order, by one block
__global__ __launch_bounds__(256) void k_head_act_param_grad(const float* __restrict__ part, int64_t n, float* __restrict__ grad) {
    __shared__ float s[256];
    float t = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) t += part[i];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) grad[0] = s[0];
}
