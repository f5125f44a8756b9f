// pair_bodies.inc -- what the pair head on M rows (pair_head.hip) and on a factored batch (pair_factored.hip) both run, each defined once.
// Included inside the anonymous namespace of both units, behind fn_internal.h and their `using fni::fail`.  As in shared_bodies.inc, no
// __global__ function may live here: one that is no template would be compiled into both.  The orders of additions that the models'
// "bitwise reproducible step" tests rest on are written HERE for v = W1^T w2 (pair_v) and the last workgroup's dW2 / db2 / loss sums
// (pair_last_tail).  Two more are the same statements in both units and stay written in each kernel, because as a shared function they
// compile to other instructions (profiles/pair_bodies_equivalence.txt section 2): the tile-row dot with w2 (k_pair_fwd | k_pairf_fwd)
// and the end of a dW1 column block (k_pair_bwd | k_pairf_bwd).  A change to one copy of those goes into the other.
constexpr int kIn0 = 256, kHid = 128;

// one 16-k step of both accumulators; !ok: this lane's quarter of the step lies behind the row's end
__device__ __forceinline__ void pair_step(const float* xp, const float* wp0, const float* wp1, bool ok, f32x4& acc0, f32x4& acc1) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 a = ok ? ld4(xp) : z, p = ok ? ld4(wp0) : z, q = ok ? ld4(wp1) : z;
    DN_MFMA(acc0, a.x, p.x);  DN_MFMA(acc1, a.x, q.x);
    DN_MFMA(acc0, a.y, p.y);  DN_MFMA(acc1, a.y, q.y);
    DN_MFMA(acc0, a.z, p.z);  DN_MFMA(acc1, a.z, q.z);
    DN_MFMA(acc0, a.w, p.w);  DN_MFMA(acc1, a.w, q.w);
}

// v[k] of v = W1^T w2: the sum over c, in order, of w2[c] W1[c, k]; W1's rows are LD long
template <int LD> __device__ __forceinline__ float pair_v(const float* __restrict__ w2, const float* __restrict__ W1, int k) {
    float v = 0.f;
#pragma unroll 8
    for (int c = 0; c < kHid; ++c) v = fmaf(w2[c], W1[(size_t)c * LD + k], v);
    return v;
}
template <int K1> constexpr int kPairColBlocks = (kIn0 + K1 + 15) / 16;      // workgroups of 16 columns of [drug | second]

// the backward of the ReLU that produced x: o where x > 0, else 0
__device__ __forceinline__ float4 relu_gate4(float4 o, float4 x) {
    return make_float4(x.x > 0.f ? o.x : 0.f, x.y > 0.f ? o.y : 0.f, x.z > 0.f ? o.z : 0.f, x.w > 0.f ? o.w : 0.f);
}

// the end of the last workgroup (256 threads = 8 row lanes x 32 float4 columns, `acc` this thread's partial of dW2): the eight partial rows
// go through sm and column t < 128 adds them ((0 + 1) + 2) + .. + 7; wave 0 sums db2 = sum_m g[m] (lane's m, m + 64, .. in order, then
// the butterfly 32 .. 1) into s1[0], wave 3 the forward's loss partials the same way (loss != null); dW2[t] = fin(sum, t, db2),
// db1[t] = w2[t] db2.
template <class Fin>
__device__ __forceinline__ void pair_last_tail(float4 acc, float* sm, float* s1, const float* __restrict__ g, int M, const float* __restrict__ w2,
                                               const float* __restrict__ loss_part, int n_part, float* __restrict__ loss, float* __restrict__ db1,
                                               float* __restrict__ dW2, float* __restrict__ db2, Fin fin) {
    const int t = threadIdx.x;
    st4(sm + 4 * ((t >> 5) * 32 + (t & 31)), acc);
    const int lane = t & 63, wv = t >> 6;                         // named behind the store: the kernels' listings follow the statement order
    if (wv == 0) {                                                // db2
        float s = 0.f;
        for (int m = lane; m < M; m += 64) s += g[m];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) s1[0] = s;
    }
    if (wv == 3 && loss) {                                        // the loss value: the forward left its partials
        float s = 0.f;
        for (int i = lane; i < n_part; i += 64) s += loss_part[i];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) loss[0] = s;
    }
    __syncthreads();
    if (t < kHid) {
        float s = sm[t];
        for (int q = 1; q < 8; ++q) s += sm[q * kHid + t];
        dW2[t] = fin(s, t, s1[0]);
        db1[t] = w2[t] * s1[0];
    }
    if (t == 0) db2[0] = s1[0];
}

// ---- host side: `who` is the entry point's name in fn_last_error(), `family` the two units' "pair_*_f32" / "pair_factored_*"
int fail_at(int code, const char* who, const char* what) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return fail(code, msg);
}
template <int K1> int check_widths(const char* family, int64_t Kd, int64_t K, int64_t H, int64_t C) {
    if (Kd == kIn0 && K == K1 && H == kHid && C == 1) return 0;
    char msg[200];
    snprintf(msg, sizeof(msg), "fn_%s_%s: the pair head is 256 + %d -> 128 -> 1 (%s, H = 128, C = 1); other widths are not built",
             K1 == 256 ? "cdrp" : "dta", family, K1, K1 == 256 ? "Kd = Kc = 256" : "Kd = 256, Kx = 300");
    return fail(FN_EUNSUPPORTED, msg);
}
// no rows / no pairs: the sums of the four parameter gradients and of the loss are empty
template <int K1> int zero_param_grads(float* dW1, float* db1, float* dW2, float* db2, float* loss, fn_stream_t stream, const char* where) {
    FN_TRY(zero_async(dW1, kHid * (kIn0 + K1), stream, where));
    FN_TRY(zero_async(db1, kHid, stream, where));
    FN_TRY(zero_async(dW2, kHid, stream, where));
    FN_TRY(zero_async(db2, 1, stream, where));
    if (loss) FN_TRY(zero_async(loss, 1, stream, where));
    return 0;
}
