// attn_readout.hip -- the attention read-out of an evaluation pass of the engine (fn_encoder_forward_attn): the last layer's
// scatter_add(attn_probs, source) of the four levels (gat2.py:165, 219, 268, 312; what fragnet/vizualize/model.py hands to viz.py) as
// ONE launch behind the last level.  The pass itself is encoder.hip's; this unit holds the one kernel it adds and its launcher
// (fni::launch_attn_readout), so that no kernel of another unit is compiled with a new caller beside it.
//
// attn[s][h] = sum_k |p[h * m + dpos_s[beg_s + k]]|, k ascending: the by-source CSR lists a source's items by ascending original edge
// id (the atom level's self loops, items m_real + i, behind its bonds), which is the order the reference's sequential scatter_add_
// adds them in -- the sums are reproducible bit for bit, and equal to k_attn_by_src's (fn_attn_by_src_f32) on the same probabilities.
// The probabilities are the evaluation launches' signed ones (sign bit = LeakyReLU branch, hence fabsf), head-major [H][m].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fn_internal.h"

namespace {
using fni::AttnReadoutTask;

constexpr int kReadoutLevels = 4;
struct ReadoutLevel {
    const int32_t* rowptr_s;      // by-source CSR: n + 1 words, positions are rowptr_s[.] - pos_base_s
    const int32_t* dpos_s;        // by-source position -> destination-order position (where p holds the item)
    const float* p;               // [H][m]
    float* out;                   // [n][H]
    const int32_t* n_real;        // nullable device word: sources at or behind *n_real are padding (0, nothing read)
    int pos_base_s, n, m;
    int64_t first;                // the level's first item in the launch's flat (level, source, head) index space
};
struct ReadoutTable {
    ReadoutLevel t[kReadoutLevels];
    int n;
    int64_t total;
};

// one thread per (level, source row, head).  Four items per trip, every load of a trip issued before the first use and none of them in
// a branch (positions clamped into the source's own segment, or to 0 for a source without items; results masked): gat_fwd.inc:77-80
template <int H>
__global__ __launch_bounds__(kBlock) void k_attn_readout(ReadoutTable T) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.total; i += (int64_t)gridDim.x * blockDim.x) {
        int ti = 0;
        while (ti + 1 < T.n && i >= T.t[ti + 1].first) ++ti;
        const ReadoutLevel& L = T.t[ti];
        const int64_t li = i - L.first;
        if (L.m == 0) { L.out[li] = 0.f;  continue; }       // a level without items: nothing is read (zeroed here, not by a memset node: batch_io.hip, fn_plan_build)
        const int s = (int)(li / H), head = (int)(li % H);
        const int live = L.n_real ? *L.n_real : L.n;
        const int beg = L.rowptr_s[s] - L.pos_base_s;
        int deg = L.rowptr_s[s + 1] - L.rowptr_s[s];
        if (s >= live || beg < 0 || deg < 0 || beg + deg > L.m) deg = 0;          // (a CSR that lies outside the level: nothing is read)
        const float* __restrict__ p = L.p + (size_t)head * L.m;
        const int last = deg > 0 ? beg + deg - 1 : 0;
        float a = 0.f;
        for (int k0 = 0; k0 < deg; k0 += 4) {
            int q[4];
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int at = beg + k0 + u;
                q[u] = L.dpos_s[at < last ? at : last];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pos = q[u] < 0 ? 0 : (q[u] < L.m ? q[u] : L.m - 1);
                v[u] = p[pos];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) a = k0 + u < deg ? a + fabsf(v[u]) : a;
        }
        L.out[li] = a;
    }
}
}  // namespace

namespace fni {
int launch_attn_readout(const AttnReadoutTask* tasks, int n_tasks, int heads, hipStream_t st) {
    if (n_tasks < 0 || n_tasks > kReadoutLevels || (n_tasks > 0 && !tasks)) return fail(FN_EINVAL, "attention read-out: bad task table");
    if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return bad_heads();
    for (int i = 0; i < n_tasks; ++i) {
        const AttnReadoutTask& a = tasks[i];
        if (!a.out) continue;
        if (a.pl.n < 0 || a.pl.m < 0 || a.pl.n > (1 << 28) || a.pl.m > (1 << 28)) return fail(FN_EUNSUPPORTED, "attention read-out: level too large for 32-bit positions");
        if (a.pl.n > 0 && a.pl.m > 0 && (!a.p || !a.pl.rowptr_s || !a.pl.dpos_s)) return fail(FN_EINVAL, "attention read-out: a level without stored probabilities or by-source CSR");
    }
    ReadoutTable T{};
    for (int i = 0; i < n_tasks; ++i) {
        const AttnReadoutTask& a = tasks[i];
        if (!a.out || a.pl.n == 0) continue;                      // not wanted, or no row to write
        ReadoutLevel& L = T.t[T.n++];          // (m == 0, a level without items: its rows are zero-filled by the same launch, nothing is read)
        L = ReadoutLevel{a.pl.rowptr_s, a.pl.dpos_s, a.p, a.out, a.n_real, a.pl.pos_base_s, (int)a.pl.n, (int)a.pl.m, T.total};
        T.total += a.pl.n * heads;
    }
    if (T.n == 0) return 0;
    const dim3 grid((unsigned)flat_grid(T.total, kGridCap));
    with_const<1, 2, 4, 8>(heads, [&](auto h) { hipLaunchKernelGGL((k_attn_readout<FN_CV(h)>), grid, dim3(kBlock), 0, st, T); });
    return launch_status("attention read-out (by-source sums of the last layer's four levels)");
}
}  // namespace fni
