// geometry.hip -- what the reference's offline featuriser derives from one conformer, on a collated batch (the
// geometry half): the bond-graph edge attribute cos(theta) (fragnet/dataset/data.py:185-211 get_edge_attr_bond_graph) and the three
// pretraining targets (data.py:224-260 get_bond_angle_dhangle).  A translation unit of its own: gathers out of a position table of
// twelve bytes per atom, nothing shared with the attention or matrix kernels but the error string.
//
// With src, dst = edge_index, p the positions, u_e = (p[src] - p[dst]) / |p[src] - p[dst]|, sigma_e = u_x + u_y + u_z and
// S_a = sum of sigma_e over the bonds e with src(e) = a, in ascending e:
//   bnd_lngth[e] = |p[src] - p[dst]|^2                       (the reference keeps the SQUARED length)
//   bnd_angl[a]  = 3 S_a^2                                   (data.py:239 sums without `dim`: a scalar broadcast to a 3-vector)
//   dh_angl[e]   = S_src S_dst (3 - sigma_e^2)               (data.py:246-258 expanded; rej_neg projects with the SOURCE's vector)
//   cos[j]       = 1 for the two directions of one bond, else the clamped dot product of the unit vectors from the shared atom of
//                  bonds edge_index_bonds_graph[:, j] to their two other atoms (RDKit's GetAngleRad followed by np.cos)
// fp32 throughout, no atomics: every S_a is one lane's running sum over its molecule's bonds in edge order, so the outputs are
// bit-identical from run to run.  No guards against coincident bonded atoms beyond the clamp (the reference divides by zero there
// too; dataset.FlatMolStore refuses such coordinates).  Ids that point outside the tables are never dereferenced: their rows are NaN.
// Products and sums are NOT contracted into FMAs here: with correctly rounded division and square root every value is then the one an
// IEEE fp32 evaluation in the same order gives on the host (synth.geometry_from_positions), bit for bit.
#include <stdint.h>

#include "fn_internal.h"

#pragma clang fp contract(off)

namespace {
using fni::fail;
using fni::launch_status;

struct Vec3 { float x, y, z; };
__device__ __forceinline__ Vec3 load3(const float* __restrict__ pos, int64_t a) {
    const float* p = pos + 3 * a;
    return Vec3{p[0], p[1], p[2]};
}
__device__ __forceinline__ Vec3 diff(const Vec3& a, const Vec3& b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float norm2(const Vec3& v) { return v.x * v.x + v.y * v.y + v.z * v.z; }
__device__ __forceinline__ Vec3 unit(const Vec3& v) {
    const float n = sqrtf(norm2(v));
    return Vec3{v.x / n, v.y / n, v.z / n};
}
__device__ __forceinline__ float quiet_nan() { return __int_as_float(0x7fc00000); }

// ---- cos(theta) of every bond-graph edge: one item per edge, the two int64 index streams read coalesced, four endpoint ids and three
// positions gathered (the position table of a batch of 512 molecules is ~165 KB: it lives in L2; nothing is staged in LDS)
__global__ __launch_bounds__(256) void k_bond_cos(const float* __restrict__ pos, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                  const int64_t* __restrict__ node1, const int64_t* __restrict__ node2, int64_t N, int64_t E,
                                                  int64_t Eb, float* __restrict__ out) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < Eb; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n1 = node1[j], n2 = node2[j];
        float r = quiet_nan();
        if (n1 >= 0 && n1 < E && n2 >= 0 && n2 < E) {
            const int64_t a1 = src[n1], b1 = dst[n1], a2 = src[n2], b2 = dst[n2];
            if (a1 == b2 && b1 == a2) {
                r = 1.0f;                                   // the two directions of one bond (one-bond fragment rule, data.py:192-195)
            } else {
                int64_t c = -1, o0 = -1, o1 = -1;           // shared atom and the two others
                if (a1 == a2) { c = a1; o0 = b1; o1 = b2; }
                else if (a1 == b2) { c = a1; o0 = b1; o1 = a2; }
                else if (b1 == a2) { c = b1; o0 = a1; o1 = b2; }
                else if (b1 == b2) { c = b1; o0 = a1; o1 = a2; }
                if (c >= 0 && c < N && o0 >= 0 && o0 < N && o1 >= 0 && o1 < N) {
                    const Vec3 pc = load3(pos, c);
                    const Vec3 u0 = unit(diff(load3(pos, o0), pc)), u1 = unit(diff(load3(pos, o1), pc));
                    const float d = u0.x * u1.x + u0.y * u1.y + u0.z * u1.z;
                    r = fminf(1.0f, fmaxf(-1.0f, d));
                }
            }
        }
        out[j] = r;
    }
}

// ---- the three pretraining targets: one workgroup per molecule.  A collated batch keeps a molecule's atoms and its directed bonds
// contiguous and in molecule order, so four binary searches (lanes 0-3) of the sorted atom -> molecule vector give the molecule's atom
// and bond ranges.  Pass 1 (a lane per bond): squared length out, sigma_e and the local source atom into LDS.  Pass 2 (a lane per
// atom): walks the molecule's bonds in edge order -- every lane reads the same LDS word, a broadcast -- and adds the sigma of its own;
// O(atoms x bonds) compares per molecule, tens x a hundred for a drug-like one.  Pass 3 (a lane per bond): dh_angl from S in LDS.
constexpr int kGeomAtoms = FN_GEOM_MAX_ATOMS, kGeomBonds = FN_GEOM_MAX_BONDS;
constexpr unsigned short kNoAtom = 0xffff;

__device__ __forceinline__ int64_t first_atom_of(const int64_t* __restrict__ atom_mol, int64_t N, int64_t m) {
    int64_t lo = 0, hi = N;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (atom_mol[mid] < m) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t first_bond_of(const int64_t* __restrict__ src, const int64_t* __restrict__ atom_mol, int64_t N, int64_t E,
                                                 int64_t m) {
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t s = src[mid];
        if (s >= 0 && s < N && atom_mol[s] < m) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_pretrain_geometry(const float* __restrict__ pos, const int64_t* __restrict__ src,
                                                           const int64_t* __restrict__ dst, const int64_t* __restrict__ atom_mol, int64_t N,
                                                           int64_t E, int64_t B, float* __restrict__ bnd_lngth, float* __restrict__ bnd_angl,
                                                           float* __restrict__ dh_angl) {
    __shared__ float s_sigma[kGeomBonds];
    __shared__ float s_S[kGeomAtoms];
    __shared__ unsigned short s_src[kGeomBonds];
    __shared__ int64_t s_rng[4];
    const int tid = threadIdx.x;
    for (int64_t m = blockIdx.x; m < B; m += gridDim.x) {
        if (tid < 2) s_rng[tid] = first_atom_of(atom_mol, N, m + tid);
        else if (tid < 4) s_rng[tid] = first_bond_of(src, atom_mol, N, E, m + (tid - 2));
        __syncthreads();
        const int64_t a0 = s_rng[0], na = s_rng[1] - a0, e0 = s_rng[2], ne = s_rng[3] - e0;
        if (na > kGeomAtoms || ne > kGeomBonds) {           // larger than the caller stated: nothing is staged, the rows say so
            for (int64_t e = tid; e < ne; e += blockDim.x) bnd_lngth[e0 + e] = dh_angl[e0 + e] = quiet_nan();
            for (int64_t a = tid; a < na; a += blockDim.x) bnd_angl[a0 + a] = quiet_nan();
            __syncthreads();
            continue;
        }
        for (int e = tid; e < (int)ne; e += blockDim.x) {
            const int64_t s = src[e0 + e], d = dst[e0 + e];
            float l2 = quiet_nan(), sg = 0.f;
            unsigned short ls = kNoAtom;
            if (s >= a0 && s < a0 + na && d >= 0 && d < N) {
                const Vec3 v = diff(load3(pos, s), load3(pos, d));
                l2 = norm2(v);
                const Vec3 u = unit(v);
                sg = (u.x + u.y) + u.z;
                ls = (unsigned short)(s - a0);
            }
            bnd_lngth[e0 + e] = l2;
            s_sigma[e] = sg;
            s_src[e] = ls;
        }
        __syncthreads();
        for (int a = tid; a < (int)na; a += blockDim.x) {
            float S = 0.f;
            for (int e = 0; e < (int)ne; ++e)
                if (s_src[e] == a) S += s_sigma[e];         // ascending edge id: the reference's masked-select order
            s_S[a] = S;
            bnd_angl[a0 + a] = 3.0f * (S * S);
        }
        __syncthreads();
        for (int e = tid; e < (int)ne; e += blockDim.x) {
            const int64_t d = dst[e0 + e] - a0;
            const unsigned short ls = s_src[e];
            float r = quiet_nan();
            if (ls != kNoAtom && d >= 0 && d < na) {
                const float sg = s_sigma[e];
                r = (s_S[ls] * s_S[d]) * (3.0f - sg * sg);
            }
            dh_angl[e0 + e] = r;
        }
        __syncthreads();                                    // the next molecule of this workgroup overwrites the staging
    }
}
}  // namespace

extern "C" {

int fn_bond_cos_f32(const float* pos, const int64_t* edge_index, const int64_t* edge_index_bonds_graph, int64_t N, int64_t E, int64_t Eb,
                    float* out, fn_stream_t stream) {
    if (N < 0 || E < 0 || Eb < 0 || N >= (1ll << 31) - 1 || E >= (1ll << 31) - 1)
        return fail(FN_EINVAL, "fn_bond_cos_f32: negative size, or more than 2^31 - 2 atoms / bonds");
    if (Eb == 0) return 0;
    if (!pos || !edge_index || !edge_index_bonds_graph || !out || (((uintptr_t)pos | (uintptr_t)out) & 3) ||
        (((uintptr_t)edge_index | (uintptr_t)edge_index_bonds_graph) & 7))
        return fail(FN_EINVAL, "fn_bond_cos_f32: null or misaligned buffer");
    hipLaunchKernelGGL(k_bond_cos, dim3(flat_grid(Eb, kGridCap)), dim3(kBlock), 0, S(stream), pos, edge_index, edge_index + E,
                       edge_index_bonds_graph, edge_index_bonds_graph + Eb, N, E, Eb, out);
    return launch_status("fn_bond_cos_f32");
}

int fn_pretrain_geometry_f32(const float* pos, const int64_t* edge_index, const int64_t* atom_mol, int64_t N, int64_t E, int64_t B,
                             int64_t max_atoms, int64_t max_bonds, float* bnd_lngth, float* bnd_angl, float* dh_angl, fn_stream_t stream) {
    if (N < 0 || E < 0 || B < 0 || max_atoms < 0 || max_bonds < 0 || N >= (1ll << 31) - 1 || E >= (1ll << 31) - 1)
        return fail(FN_EINVAL, "fn_pretrain_geometry_f32: negative size, or more than 2^31 - 2 atoms / bonds");
    if (max_atoms > FN_GEOM_MAX_ATOMS || max_bonds > FN_GEOM_MAX_BONDS)
        return fail(FN_EUNSUPPORTED, "fn_pretrain_geometry_f32: a molecule of more than FN_GEOM_MAX_ATOMS (1024) atoms or FN_GEOM_MAX_BONDS "
                                     "(4096) directed bonds does not fit the per-molecule staging");
    if (N == 0 || B == 0) {
        if (E > 0) return fail(FN_EINVAL, "fn_pretrain_geometry_f32: bonds without atoms or molecules");
        return 0;
    }
    if (!pos || !atom_mol || !bnd_angl || (E > 0 && (!edge_index || !bnd_lngth || !dh_angl)) ||
        (((uintptr_t)pos | (uintptr_t)bnd_lngth | (uintptr_t)bnd_angl | (uintptr_t)dh_angl) & 3) ||
        (((uintptr_t)edge_index | (uintptr_t)atom_mol) & 7))
        return fail(FN_EINVAL, "fn_pretrain_geometry_f32: null or misaligned buffer");
    const unsigned grid = (unsigned)(B < (1 << 20) ? B : (1 << 20));
    hipLaunchKernelGGL(k_pretrain_geometry, dim3(grid), dim3(256), 0, S(stream), pos, edge_index, edge_index + E, atom_mol, N, E, B, bnd_lngth,
                       bnd_angl, dh_angl);
    return launch_status("fn_pretrain_geometry_f32");
}

}  // extern "C"
