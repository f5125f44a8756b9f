// row_masks.hip -- fn_loo_row_masks_u8: the three byte masks of a batch of leave-one-out replicas (fn_encoder_forward_masked reads them),
// zero-filled and set in one launch.  A thread owns 16 consecutive rows of one index space -- one 16-byte store -- finds the molecule of
// its first row by bisection in that space's offsets and walks on from there: a molecule is a few dozen rows, so a thread crosses at
// most a handful of molecule boundaries.
#include "fn_internal.h"

namespace {
using fni::fail;
using fni::launch_status;

struct RowMaskArgs {
    const int32_t* replicas;      // [n_mols][2]: kind, local index
    int n_mols;
    const int32_t* off[3];        // [n_mols + 1] per space: atoms, directed bonds, directed fragment connections
    uint8_t* mask[3];
    int n[3];                     // rows per space
    int chunk0[4];                // first 16-row chunk of each space in the launch's flat chunk index; [3] = all chunks
    int32_t* status;
};

// is row r (local to its molecule, which has cnt rows in this space) masked by the molecule's replica?
__device__ __forceinline__ bool row_hit(int space, int kind, int idx, int r, int cnt) {
    if (kind != space + 1 || idx < 0) return false;
    if (space == 0) return idx < cnt && r == idx;
    return 2 * (int64_t)idx + 1 < cnt && (r >> 1) == idx;          // both directed rows of the pair, and only if both exist
}

__global__ __launch_bounds__(kBlock) void k_loo_row_masks(RowMaskArgs A) {
    const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    // the replicas' own range check: one thread per molecule (the first n_mols threads of the launch)
    if (g < A.n_mols) {
        const int kind = A.replicas[2 * g], idx = A.replicas[2 * g + 1];
        bool bad = kind < 0 || kind > 3;
        if (!bad && kind > 0) {
            const int cnt = A.off[kind - 1][g + 1] - A.off[kind - 1][g];
            bad = idx < 0 || (kind == 1 ? idx >= cnt : 2 * (int64_t)idx + 1 >= cnt);
        }
        if (bad) atomicOr(A.status, FN_STATUS_BAD_REPLICA);
    }
    if (g >= A.chunk0[3]) return;
    const int space = g >= A.chunk0[2] ? 2 : (g >= A.chunk0[1] ? 1 : 0);
    const int row0 = (g - A.chunk0[space]) * 16, n = A.n[space];
    const int32_t* __restrict__ off = A.off[space];
    // molecule of row0: the last m with off[m] <= row0 (molecules without rows in this space share an offset: the walk below skips them)
    int lo = 0, hi = A.n_mols;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= row0) lo = mid; else hi = mid;
    }
    int m = lo, m_beg = off[m], m_end = off[m + 1];
    int kind = A.replicas[2 * m], idx = A.replicas[2 * m + 1];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int r = row0 + i;
        while (r >= m_end && m + 1 < A.n_mols) {
            ++m;  m_beg = m_end;  m_end = off[m + 1];
            kind = A.replicas[2 * m];  idx = A.replicas[2 * m + 1];
        }
        const bool hit = r < n && r < m_end && row_hit(space, kind, idx, r - m_beg, m_end - m_beg);
        w[i >> 2] |= (hit ? 1u : 0u) << (8 * (i & 3));
    }
    uint8_t* dst = A.mask[space] + row0;
    if (row0 + 16 <= n) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else
        for (int i = 0; row0 + i < n; ++i) dst[i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);      // the space's last, partial chunk
}
}  // namespace

extern "C" {
int fn_loo_row_masks_u8(const int32_t* replicas, int64_t n_mols, const int32_t* atom_off, const int32_t* bond_off,
                        const int32_t* fbond_off, uint8_t* mask_atoms, int64_t N, uint8_t* mask_bonds, int64_t E,
                        uint8_t* mask_fbonds, int64_t EF, int32_t* status, fn_stream_t stream) {
    if (!replicas || !atom_off || !bond_off || !fbond_off || !status) return fail(FN_EINVAL, "fn_loo_row_masks_u8: null argument");
    if (n_mols < 1 || n_mols > (1 << 24)) return fail(FN_EINVAL, "fn_loo_row_masks_u8: n_mols out of range");
    if (N < 0 || E < 0 || EF < 0 || N > (1 << 30) || E > (1 << 30) || EF > (1 << 30)) return fail(FN_EINVAL, "fn_loo_row_masks_u8: row counts out of range");
    if ((N && !mask_atoms) || (E && !mask_bonds) || (EF && !mask_fbonds)) return fail(FN_EINVAL, "fn_loo_row_masks_u8: null mask array");
    if (((uintptr_t)mask_atoms | (uintptr_t)mask_bonds | (uintptr_t)mask_fbonds) & 15) return fail(FN_EINVAL, "fn_loo_row_masks_u8: mask arrays must be 16-byte aligned");
    RowMaskArgs A{};
    A.replicas = replicas;  A.n_mols = (int)n_mols;  A.status = status;
    A.off[0] = atom_off;  A.off[1] = bond_off;  A.off[2] = fbond_off;
    A.mask[0] = mask_atoms;  A.mask[1] = mask_bonds;  A.mask[2] = mask_fbonds;
    A.n[0] = (int)N;  A.n[1] = (int)E;  A.n[2] = (int)EF;
    int64_t chunks = 0;
    for (int s = 0; s < 3; ++s) { A.chunk0[s] = (int)chunks;  chunks += (A.n[s] + 15) / 16; }
    A.chunk0[3] = (int)chunks;
    const int64_t threads = chunks > n_mols ? chunks : n_mols;
    hipLaunchKernelGGL(k_loo_row_masks, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, S(stream), A);
    return launch_status("fn_loo_row_masks_u8");
}
}  // extern "C"
