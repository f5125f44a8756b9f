// Internal declarations shared by the translation units of libfragnet_hip.so (not part of the C-ABI: nothing here is exported).
//  * device helpers every kernel file uses (vector loads, DPP reductions inside a head's lanes, Philox);
//  * the per-molecule extents table (MolExt) the molecule-resident kernels are driven by;
//  * host-side hooks (namespace fni): the error string and the tuning table, which live in fragnet_hip.hip, and the launchers one unit
//    offers the others.  A hook's signature is made of C-ABI and fni:: types only: a type of a unit's unnamed namespace has no linkage
//    to carry across units (the kernel argument blocks that stay unnamed -- GatBwdDstArgs, RowDotsBwdArgs, .. -- therefore travel as
//    plain arguments, or the code that fills them is in an .inc both units include).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "fragnet_hip.h"

#define FNI_HIDDEN __attribute__((visibility("hidden")))

namespace fni {
FNI_HIDDEN int fail(int code, const char* what);        // sets fn_last_error(), returns code
FNI_HIDDEN int launch_status(const char* where);        // hipGetLastError() -> 0 / error code + message
FNI_HIDDEN int tune(int key);                           // fn_set_tuning table
FNI_HIDDEN unsigned long long* stamps(int64_t* n_u64);  // fn_debug_set_stamps buffer (null: none)

// extents of one molecule in the index spaces of a collated batch (dataset/data.py:877-948 concatenates molecules, so every
// one of these is a contiguous range); filled by k_mol_extents from the molecule CSRs and the level plans
struct MolExt {
    int a0, na;            // atoms
    int b0, nb;            // directed bonds = bond-graph nodes = atom-graph edges
    int f0, nf;            // fragments
    int c0, nc;            // fragment connections = fragment-bond-graph nodes = fragment-graph edges
    int eb0, meb;          // bond-graph edges: level-local destination-sorted positions
    int ea0, mea;          // atom-graph items (edges + self loops)
    int ef0, mef;          // fragment-bond-graph edges
    int ec0, mec;          // fragment-graph items
};
static_assert(sizeof(MolExt) == 64, "MolExt is sixteen int32 (include/fragnet_hip.h documents it as int32 [n_mols][16])");

// ---- argument blocks and host-side entry points shared by the translation units, grouped by the unit that defines them: the forward
// attention family in gat_fwd.hip / gat_fwd_lin.hip, the one-pass attention backward in gat_bwd_one.hip, the operator surface (and the
// grouped projection launches) in fragnet_hip.hip, the parameter-gradient queue in param_grads.hip.  The engine, encoder.hip, offers
// nothing here: it is the caller of all of them, and
// besides these hooks it calls the C-ABI's own single-operator entry points where a level or variant runs them one by one
// (fn_gat_bwd_dst_f32, fn_gat_fwd_f32, fn_node_scalars_f32, fn_row_dots_sorted_f32, fn_dropout_act_f32, fn_linear128_f32,
// fn_segment_sum_f32).
struct GatFwdArgs {
    const float *h, *s_dst, *s_src, *att;
    int att_w;
    fn_edge_term et;
    fn_gat_plan pl;
    float slope;
    float *out, *p_sorted, *probs_orig;
    fn_act_epilogue ep;
    int rows_per_hw, nblk;
    // optional fused "row dots" of the level that consumes this one's raw output as its edge attribute (bond graph -> atom
    // graph, gat2.py:203-208): rd_out[j * rd_m + rd_pos[t]] = <out[t, :], rd_A[j * rd_lda : +128]>, j < rd_J -- the edge term
    // of the next level, written straight into ITS destination-sorted order (rd_pos = that level's inv_d)
    const float* rd_A;
    float* rd_out;
    const int32_t* rd_pos;
    int64_t rd_m;
    int rd_lda, rd_J;
    // optional second output for the one-pass backward (gat_bwd_one.inc): out2[t] = sum_e lambda_e p_e h[src_e] and
    // sigma[t, h] = sum_e lambda_e p_e, lambda_e = 1 where z_e > 0, else the LeakyReLU slope
    float *out2, *sigma;
    int p_edge_major;     // p_sorted as [m][H] instead of [H][m]: what the one-pass backward gathers by position (one line per edge)
    const int32_t* n_real;   // nullable device word: rows >= *n_real are padding (zero outputs, nothing gathered)
    int tier6;               // gather tiers 4 / 6 / 8 (1) or 4 / 8 (0)
};
struct NodeScalarEpi {             // optional fused epilogue: s_dst/s_src[row, head] = <Y[row, head cols], att blocks>
    const float* att;
    float* s_dst;
    float* s_src;
    int att_w, dst_off, src_off, heads;     // heads in {2, 4, 8}: a head's columns must lie inside one wave's 64
};
struct RowAdd {
    const float* z;           // [M][4]: dL/d(edge term) of row e, the four heads together; null: no term
    const float* a;           // a[h * lda + column]
    int lda;
};
struct CuEpi {
    const float *out, *out2, *sigma;
    float *c, *u;             // c == null: no such epilogue
    int heads;
};
// up to three independent [M_i,K]·[K,128] products in one launch: the three projections of a layer (forward) or
// their three input-gradient products (backward) depend only on the previous layer, never on each other
struct LinTask {
    const float* Wn;          // the same weight n-major ([128 n][K]) for k_proj128; null: only the k_linear128 form is available
    const float *X, *Bt, *bias;
    float* Y;
    int64_t M;
    fn_act_epilogue mk;
    NodeScalarEpi ns;
    int first, nblk;
    int K;                    // 0: the group's K (LinTasks::K); else this task's own reduction length (layer 0: 17 bond / 6 connection features)
    RowAdd ra;                // riding input-gradient products only (lin_side_block)
    CuEpi cu;                 // ... of the one-pass backward (lin_side_block<true>)
    const int32_t* n_real;    // nullable device word: row tiles that start at or behind *n_real are padding and are not computed
};
struct LinTasks {
    LinTask t[3];
    int n, K;
    int base, total;          // co-launched with an attention pass (below): the GEMM workgroups are blocks [base, base + total) of that launch
};
// gat_fwd.hip
FNI_HIDDEN int prep_gat_fwd(const float* h, const float* s_dst, const float* s_src, const float* att, int att_w, const fn_edge_term* et,
                            const fn_gat_plan* plan, float neg_slope, float* out, float* p_sorted, float* probs_orig,
                            const fn_act_epilogue* act, int heads, GatFwdArgs* A, float* out2 = nullptr, float* sigma = nullptr);
// A non-null FwdMask makes a launch a MASKED evaluation launch (forward kind 4, gat_fwd.inc): rows[t] != 0 -> row t of the level is zero
// for everything that reads it.  rows == null: a level of a masked pass that has no mask of its own.  In a two-level launch both come or neither.
struct FwdMask { const uint8_t* rows; };
FNI_HIDDEN int launch_gat_fwd(const GatFwdArgs& A, int heads, hipStream_t st, const FwdMask* mk = nullptr);
FNI_HIDDEN int launch_gat_fwd_pair(const GatFwdArgs& A, const GatFwdArgs& B, int heads, hipStream_t st, const FwdMask* mka = nullptr, const FwdMask* mkb = nullptr);
// gat_fwd_lin.hip: an attention pass + the K = 128 projection tiles that do not depend on it, in one launch
FNI_HIDDEN int launch_gat_fwd_lin(const GatFwdArgs& A, LinTasks& T, int heads, hipStream_t st, const FwdMask* mk = nullptr);
FNI_HIDDEN int launch_gat_fwd_pair_lin(const GatFwdArgs& A, const GatFwdArgs& B, LinTasks& T, int heads, hipStream_t st, const FwdMask* mka = nullptr,
                                       const FwdMask* mkb = nullptr);
// ---- the one-pass attention backward (gat_bwd_one.hip / gat_bwd_one.inc)
struct GatBwdOneArgs {
    const float *g_out, *h, *p_sorted, *cdot, *g_s_dst, *att;
    int att_w, dst_off, src_off;
    fn_edge_term et;
    fn_gat_plan pl;
    float slope;
    float *g_h, *part_a, *part_e, *dz_sorted, *g_s_orig;
    int rows_per_hw, nblk;
    int p_edge_major;       // p_sorted is [m][H] (the engine's forward writes it so: one cache line per edge) instead of [H][m]
    const float* x_src;     // mode 2, nullable: the raw attribute [K][m] in SOURCE order (streamed) instead of gathers from et.x_sorted
    const int32_t* n_real;        // nullable device word: source rows >= *n_real are padding (zero gradient row out, nothing gathered)
    int tier6;                    // gather tiers 4 / 6 / 8 / 12 (1) or 4 / 8 / 12 (0)
    float* dz_em;                 // operator-level deferred form (fn_gat_bwd_one_f32 only; the engine leaves it null): dL/dz of every edge at its destination-order slot, EDGE-major [m][H]
    unsigned long long* stamps;   // dev aid (fn_debug_set_stamps): 16 s_memtime values per wave -- entry, loop start, per row (loads issued,
                                  // data arrived, row done) x 4, loop end, exit; null in production (one uniform branch per stamp)
    int part_ld;                  // layout of part_a (part_at, below): 0 = column-major [256][FN_MAX_PART] (the operator entry points), else the
                                  // leading dimension of row-major [nblk][part_ld] (the engine's tables)
};
struct CuTask {
    const float *g, *out, *out2, *sigma;
    float scale;
    float *c, *u;
    int64_t n;
    int first, nblk;
};
constexpr int kMaxCuTasks = 4;
struct CuTasks { CuTask t[kMaxCuTasks]; int n; };
struct GsdSegTask {
    const float* dz;          // [m][4]
    const int32_t* rowptr;    // by-destination CSR, n + 1 words; positions are rowptr[.] - pos_base
    int pos_base;
    int64_t n;
    float* gsd;               // out [n][4]
    const int32_t* n_real;    // nullable: rows at or behind *n_real are padding (their segments were never written): zeros
    const float* h;           // [n][128] the level's projected rows
    float* part_a;            // column-major [2 * 128][FN_MAX_PART]: columns 0..127, rows 0..nblk-1 are written
    int first, nblk;
};
struct GsdSegTasks { GsdSegTask t[3]; int n; };
FNI_HIDDEN int prep_gat_bwd_one(const float* g_out, const float* h, const float* p_sorted, const float* cdot, const float* g_s_dst,
                                const fn_edge_term* et, const float* att, int att_w, int dst_off, int src_off, const fn_gat_plan* plan,
                                float neg_slope, float* g_h, float* dz_sorted, float* g_s_orig, float* part_a, int* n_part_a, float* part_e,
                                int* n_part_e, int heads, GatBwdOneArgs* A);
FNI_HIDDEN int launch_gat_bwd_one(const GatBwdOneArgs& A, int heads, hipStream_t st);
FNI_HIDDEN int launch_gat_bwd_one3(const GatBwdOneArgs& A, const GatBwdOneArgs& B, const GatBwdOneArgs& C, int heads, hipStream_t st);
FNI_HIDDEN int launch_gat_cu(CuTasks& T, int heads, hipStream_t st);
FNI_HIDDEN int launch_gsd_seg(const GsdSegTasks& T, int blocks, hipStream_t st);
// fragnet_hip.hip
FNI_HIDDEN int launch_linear128_group(LinTasks& T, hipStream_t st);           // up to three K = 128 products (k_linear128_multi / _multi_ra)
FNI_HIDDEN int launch_linear128_small_group(LinTasks& T, hipStream_t st);     // layer 0's raw-feature projections, each task with its own K <= 168
// fn_linear128_f32 with the node scalars of the attention level it feeds as its epilogue (ns.att == null: fn_linear128_f32 itself)
FNI_HIDDEN int launch_linear128_ns(const float* X, int K, const float* Bt, const float* bias, float* Y, int64_t M, const fn_act_epilogue* act_bwd,
                                   NodeScalarEpi ns, fn_stream_t stream);
// out[i, :] = table[index[i], :] (+ addend[i, :], which may alias out), rows of w4 float4 (k_gather_rows4); where: the launch's name in fn_last_error()
FNI_HIDDEN int launch_gather_rows4(const float* table, const int64_t* index, float* out, int64_t rows, int64_t w4, const float* addend, hipStream_t st,
                                   const char* where);
// attn_readout.hip: the by-source sums of stored probabilities (p: signed, head-major [H][m]) of up to four levels in ONE launch --
// out[s][h] = sum over the items of source s, in by-source order, of |p[h][.]|.  A task without `out` is skipped, a level without
// items zero-fills its rows; n_real: nullable device word, sources at or behind it are padding (0)
struct AttnReadoutTask {
    fn_gat_plan pl;
    const float* p;
    float* out;               // [pl.n][heads]
    const int32_t* n_real;
};
FNI_HIDDEN int launch_attn_readout(const AttnReadoutTask* tasks, int n_tasks, int heads, hipStream_t st);
// input_grad.hip: up to FN_MAX_DX_TASKS products dx = g W (+ row dots with a caller table) in ONE launch; fn_linear_dx_f32 itself
FNI_HIDDEN int launch_linear_dx(const fn_linear_dx_task* tasks, int n_tasks, hipStream_t st);
// ---- param_grads.hip: the parameter-gradient family.  A backward pass leaves per-block partials behind (attention-vector and
// edge-embedding partials of each level, the edge term's column sums, the weight-gradient partials) and queues a task per reduction; the
// queue launches the grouped weight-gradient partial products and then ONE kernel for all reductions (k_reduce_tasks).  The argument
// blocks of those kernels:
enum { RT_FINALIZE = 0, RT_COLSUM = 1, RT_WGRAD = 2 };
struct ReduceTask {
    int kind, first, nblk, H;
    const float *p0, *p1;
    int n0, n1;
    fn_edge_term et;
    const float* att;
    int att_w, dst_off, src_off, K;
    float *o0, *o1, *o2;
    int ld, off, cls, pld;       // cls (RT_WGRAD): the class of the kernel that wrote the partials (param_grads.hip: wgrad_class)
                                 // pld (RT_FINALIZE: p0, RT_COLSUM): layout of the partials, as part_at takes it (0: column-major)
};
constexpr int kMaxReduceTasks = 36;      // one launch for all 30 tasks of a 4-layer backward pass (5.5 KB of kernel arguments)
struct ReduceTasks {
    ReduceTask t[kMaxReduceTasks];
    int first[kMaxReduceTasks + 1];      // first block of every task, packed: a block finds its task by walking THIS array (three
                                         // cache lines of the argument block) -- walking t[].first was one dependent scalar load
                                         // per 152-byte struct, up to 30 in a row from the kernel-argument segment: 10 of the
                                         // launch's 22 us before the first partial was read
    int n;
};
struct WgradTask {
    const float *dY, *X;
    float* part;
    int64_t M;
    int rpb, first;
    int K;                    // k_linear128_wgrad_mixed only: this product's reduction length (0 elsewhere: WgradTasks::K)
    const int32_t* n_real;    // nullable device word: rows at or behind *n_real are padding (zero gradient rows) and are not read
};
constexpr int kMaxWgradTasks = 3 * FN_MAX_LAYERS;
struct WgradTasks {
    WgradTask t[kMaxWgradTasks];
    int n, K;
};
// what the queue's methods take: pointers and counts, nothing of the caller's own types
struct AttParamGrads {       // dL/d(attention vector [H][att_w], edge embedding) of a level from the partial rows its pass wrote
    int H;
    const float* part_a;  int n_a;      // destination / source block partials [n_a rows written][2 * 128] in the layout part_ld names
    const float* part_e;  int n_e;      // mode-2 levels: [n_e][H * (K + 1)] edge-embedding partials (else null / 0)
    fn_edge_term et;
    const float* att;  int att_w, src_off;      // the level's attention vector; destination block at 0, source block at src_off
    float *g_att, *g_embW, *g_embb;     // out (the last two: mode 2 only)
    int part_ld;                        // layout of part_a (part_at): 0 = column-major [2 * 128][FN_MAX_PART], else row-major with this leading dimension
};
struct ProjWgrad {           // dW [128][K], db [128] of a projection from its gradient rows g_h [M][128] and input rows x [M][K]
    const float *g_h, *x;
    int K;
    int64_t M;
    float* ws;                // partial workspace, fn_linear128_wgrad_ws(M, max(K, 128)) floats
    const int32_t* n_real;    // nullable device word: rows at or behind it are padding
    float *dW, *db;
};
// A stack object of a backward pass; nothing is allocated.  The settings are set once before the first task.  A flush in the middle of a
// pass (more than kMaxReduceTasks / kMaxWgradTasks queued: six or more layers) runs what is queued, so everything a queued task reads
// must have been launched on `st` before the task is queued.
struct FNI_HIDDEN ParamGradQueue {
    hipStream_t st = nullptr;               // the grouped products and the reductions run here
    bool defer_mixed = false;               // layer 0's products (K != 128) wait for a grouped launch too, instead of one launch each
    fn_adam_slice* rider = nullptr;         // fn_encoder.adam_rider: rides in the LAST deferred-reduction launch of the pass (null: none, or gone elsewhere)
    int finalize(const AttParamGrads& a);
    // out[(col / 128) * ld + off + col % 128] = sum of the n_rows written rows of column col of part (part_ld == 0: column-major
    // [cols][FN_MAX_PART]; else row-major [n_rows][part_ld])
    int colsum(const float* part, int n_rows, int cols, float* out, int ld, int off, int part_ld = 0);
    // partial product now (on `launch_on`) where it is launched alone, else with its group in flush(); reduction with the rest
    int wgrad(const ProjWgrad& p, hipStream_t launch_on);
    int flush(bool last = false);           // last: the pass's final flush, which carries the rider
private:
    ReduceTasks T{};
    WgradTasks W{}, W0{};                   // W: the K = 128 products; W0: the others (layer 0), k_linear128_wgrad_mixed
    int blocks = 0, wblocks = 0, w0blocks = 0;
    int w_reduce[kMaxWgradTasks] = {};      // index in T of each grouped product's reduction
    int push(ReduceTask t, int nblk);
    void size_group128();
    int flush_wgrad();
};
FNI_HIDDEN int prof_event(int i, hipStream_t st);                             // records event i of fn_debug_set_profile_events, if set
FNI_HIDDEN bool bad_edge_term(const fn_edge_term* et, int64_t m);
}  // namespace fni

namespace {
inline hipStream_t S(fn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
#define FN_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
// a launch with more than 64 KB of dynamic LDS has to be allowed per kernel first
template <typename Kern> inline int allow_lds(Kern kern, size_t bytes) {
    if (bytes <= 64 * 1024) return 0;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fni::fail((int)e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"); }
    return 0;
}
// n floats of zeros on the stream; where: the step's name in fn_last_error()
inline int zero_async(float* p, int64_t n, fn_stream_t stream, const char* where) {
    if (hipMemsetAsync(p, 0, (size_t)n * sizeof(float), S(stream)) != hipSuccess) return fni::launch_status(where);
    return 0;
}
// whether one of up to five pointers (null: none) has a bit of `mask` set: 3 / 7 / 15 for 4- / 8- / 16-byte alignment
inline bool misaligned(unsigned mask, const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr,
                       const void* e = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e) & mask) != 0;
}
// ---- which KIND of the attention forward (the O2 template argument of its kernels) a launch takes.  The comment above gat_fwd_rows
// (gat_fwd.inc) is the one description of what each kind takes for granted; it calls the kind 2 / kind 3 conditions below
// fwd_kind_tr() / fwd_kind_ev().  masked: the launch comes with a FwdMask; such a launch is kind 4 or does not exist (kFwdNoKind).
constexpr int kFwdNoKind = -1;
inline int fwd_kind(const fni::GatFwdArgs& A, int heads, bool masked) {
    const bool o2 = A.out2 != nullptr, drop = A.ep.p > 0.f;
    // what the kinds with compile-time flags (2, 3, 4) share: four heads, no probs_orig, probabilities edge-major with the second output
    // and head-major without, an epilogue (if any) that is a ReLU -- after dropout with the second output, without dropout otherwise --
    // and row dots (if any) of every head
    const bool flags = heads == 4 && A.probs_orig == nullptr && (A.p_edge_major != 0) == o2 &&
                       (A.ep.y == nullptr || (A.ep.relu != 0 && drop == o2)) && (A.rd_out == nullptr || A.rd_J == heads);
    if (masked) return flags && !o2 ? 4 : kFwdNoKind;                       // (a masked level may have fewer than two edges)
    if (flags && fni::tune(FN_TUNE_ENGINE_CONST) != 0 && A.pl.m >= 2) return o2 ? 2 : 3;
    return o2 ? 1 : 0;
}
inline int fwd_kind_plain(int kind) { return kind == 2 ? 1 : kind == 3 ? 0 : kind; }     // kinds 2 / 3 are kinds 1 / 0 with constant flags
// two levels in one launch run ONE kind: the kind both take, else the plain kind (0 / 1) both reduce to, else kFwdNoKind -- one level
// with the second output and one without, or a masked launch in which a level has no FwdMask or is not kind 4.  The caller then runs
// the levels one by one (unmasked) or fails (masked).
inline int fwd_kind_pair(const fni::GatFwdArgs& A, const fni::GatFwdArgs& B, int heads, const fni::FwdMask* mka, const fni::FwdMask* mkb) {
    const bool masked = mka || mkb;
    if (masked && !(mka && mkb)) return kFwdNoKind;
    const int ka = fwd_kind(A, heads, masked), kb = fwd_kind(B, heads, masked);
    if (ka == kb) return ka;
    if (masked) return kFwdNoKind;
    return fwd_kind_plain(ka) == fwd_kind_plain(kb) ? fwd_kind_plain(ka) : kFwdNoKind;
}
// ---- run-time values to template arguments: with_const<V0, V1, ..>(v, f) calls f(std::integral_constant<int, Vi>{}) for the Vi equal to
// v and returns whether there was one.  A kernel called from f is instantiated for the listed values and no others.
template <int... Vs, class F> inline bool with_const(int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
#define FN_CV(c) decltype(c)::value
template <class F> inline bool with_edge_class(int kl, F&& f) { return with_const<0, 1, FN_MAX_EDGE_K>(kl, f); }     // kl: edge_class(), below
inline int bad_heads() { return fni::fail(FN_EUNSUPPORTED, "heads must be 1, 2, 4 or 8 (128 = heads * head_dim)"); }
// (heads, kind) of an UNMASKED attention forward launch: f(H, O2).  Kinds 2 and 3 exist for four heads only (fwd_kind returns them for
// no other count); kind 4 has kernels of its own (four heads)
template <class F> inline int with_heads_kind(int heads, int kind, F&& f) {
    const bool ok = kind >= 2 ? heads == 4 && with_const<2, 3>(kind, [&](auto k) { f(std::integral_constant<int, 4>{}, k); })
                              : with_const<1, 2, 4, 8>(heads, [&](auto h) { with_const<0, 1>(kind, [&](auto k) { f(h, k); }); });
    return ok ? 0 : bad_heads();
}
// the head count of every other launch: f(H)
template <class F> inline int with_heads(int heads, F&& f) { return with_const<1, 2, 4, 8>(heads, f) ? 0 : bad_heads(); }
constexpr int kBlock = 256;
constexpr int kRows = 8;          // rows (half-waves) per block
constexpr int kGridCap = 2048;    // memory-bound kernels: ~8 blocks per CU, grid-stride the rest
constexpr int kBwdRows = 8;       // rows (half-waves) per block in the attention backward kernels
inline int row_grid(int64_t rows, int cap) {
    int64_t g = (rows + kRows - 1) / kRows;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
inline int flat_grid(int64_t work, int cap) {
    int64_t g = (work + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}
// edge class of an attention level = the KL template argument of its kernels: 0 stored edge term, 1 / FN_MAX_EDGE_K raw attributes
inline int edge_class(const fn_edge_term* et) { return et->mode == 0 ? 0 : (et->K == 1 ? 1 : FN_MAX_EDGE_K); }
// the two-level forward kernels exist for two levels that are both there, the first of edge class 1, the second of class 1 or FN_MAX_EDGE_K
inline bool fwd_pair_classes(const fni::GatFwdArgs& A, const fni::GatFwdArgs& B) {
    return A.nblk != 0 && B.nblk != 0 && edge_class(&A.et) == 1 && edge_class(&B.et) != 0;
}
inline int lin_blocks(int64_t tiles, int iters) { return 2 * (int)((tiles + iters - 1) / iters); }     // 64 x 64 tiles: two column halves per row tile
// lays the workgroups of a task group out: drops the tasks without rows, gives every other one the blocks [first, first + nblk) -- each
// walks `iters` tiles of `tile_rows` rows --, compacts T.t[] and returns the block total
inline int lin_layout(fni::LinTasks& T, int tile_rows, int iters) {
    int blocks = 0, live = 0;
    for (int i = 0; i < T.n; ++i) {
        if (T.t[i].M <= 0) continue;
        fni::LinTask t = T.t[i];
        t.first = blocks;
        t.nblk = lin_blocks((t.M + tile_rows - 1) / tile_rows, iters);
        blocks += t.nblk;
        T.t[live++] = t;
    }
    T.n = live;
    return blocks;
}

constexpr int kWfLd = FN_MAX_EDGE_K + 1;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
    acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y);
    acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}

// XCD-aware work split.  Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one, each XCD has
// its own 4 MiB L2), so logical block ids are remapped to give every XCD one CONTIGUOUS range of rows: the
// source rows a destination gathers belong to the same molecule, i.e. to neighbouring rows, and then stay
// in that XCD's L2 instead of being fetched by all eight.  Bijective for any grid size; speed only.
__device__ __forceinline__ int xcd_block(int b, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}
#ifndef FN_XCD_REAL
#define FN_XCD_REAL 1
#endif
#ifndef FN_PAD_BLOCK_EXIT
#define FN_PAD_BLOCK_EXIT 1
#endif
// Per-block partial sums of the parameter gradients (part_a, the edge term's part_rd): a table of `cols` columns and one row per
// block.  The operator entry points keep it column-major [cols][FN_MAX_PART] (ld == 0: what their callers index); the engine's own
// tables are row-major [rows][ld], so a block's 256 .. 768 values are full cache lines instead of 4-byte stores 16 KB apart.  The
// deferred reduction adds the rows of a column in the same order either way (param_grads.hip: rowmajor_sum_32).
// -DFN_PART_ROWMAJOR=0: the engine's tables are column-major too (the A/B arm; same sums bit for bit).
#ifndef FN_PART_ROWMAJOR
#define FN_PART_ROWMAJOR 1
#endif
__device__ __forceinline__ size_t part_at(int ld, int row, int col) {
    return ld ? (size_t)row * ld + col : (size_t)col * FN_MAX_PART + row;
}
// The same for a static-shape batch whose rows behind logical block `nreal` are padding.  Dealing CAPACITY blocks into eight chunks
// leaves the last XCD with mostly padding and the other seven with capacity / 8 rows each instead of real / 8 -- 8 % padding made the
// attention launches 6-9 % longer (round 4).  Here the REAL blocks [0, nreal) are dealt evenly (contiguous chunks as above) and the
// padding blocks follow behind them in (XCD, turn) order.  Bijective on [0, nwg) for any 0 <= nreal <= nwg.
__device__ __forceinline__ int xcd_block_real(int b, int nwg, int nreal) {
    if (!FN_XCD_REAL || nreal >= nwg || nreal <= 0) return xcd_block(b, nwg);
    const int x = b & 7, k = b >> 3;
    const int qr = (nreal >> 3) + (x < (nreal & 7) ? 1 : 0);          // real blocks of this XCD
    if (k < qr) return xcd_block(b, nreal);
    int before = 0;                                                    // padding blocks of the XCDs in front
#pragma unroll
    for (int y = 0; y < 7; ++y)
        if (y < x) before += ((nwg >> 3) + (y < (nwg & 7) ? 1 : 0)) - ((nreal >> 3) + (y < (nreal & 7) ? 1 : 0));
    return nreal + before + (k - qr);
}
// [begin, end) of the row groups (RB rows each) owned by this block: contiguous chunks, XCD-swizzled
__device__ __forceinline__ void block_groups(int64_t n_rows, int rb, int64_t& begin, int64_t& end) {
    const int64_t groups = (n_rows + rb - 1) / rb;
    const int64_t per = (groups + gridDim.x - 1) / gridDim.x;
    begin = (int64_t)xcd_block(blockIdx.x, gridDim.x) * per;
    end = begin + per < groups ? begin + per : groups;
}

// Philox-4x32 counter-based generator (Salmon et al., SC'11): 128 random bits per (counter, key), no state.  SEVEN rounds: the
// smallest count that passes BigCrush in the paper (Table 2; ten is its safety-margin default).  The bits only draw dropout masks,
// and the attention forward kernels are VALU-bound enough for the three rounds to matter: two 32 x 32 -> 64 multiplies (quarter
// rate) per round and lane, 1.2 % of the whole training step (0.809 -> 0.799 ms, profiles/r05_*; -DFN_PHILOX_ROUNDS=10 for the A/B).
// Every consumer of a mask -- the fused epilogues, fn_dropout_act_f32, its backward, the tests that replay masks -- calls this.
#ifndef FN_PHILOX_ROUNDS
#define FN_PHILOX_ROUNDS 7
#endif
__device__ __forceinline__ uint4 philox4x32(uint64_t ctr, uint64_t seed) {
    uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0u, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < FN_PHILOX_ROUNDS; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;       // one v_mad_u64_u32 each
        const uint32_t hi0 = (uint32_t)(m0 >> 32), lo0 = (uint32_t)m0, hi1 = (uint32_t)(m1 >> 32), lo1 = (uint32_t)m1;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// keep an element iff u >= p with u = (bits >> 8) / 2^24 -- decided on the integers: k / 2^24 >= p  <=>  k >= ceil(p 2^24) (both sides
// exact in fp32), which saves the conversion and the multiply per element; the threshold is loop-invariant
__device__ __forceinline__ float keep_scale(uint32_t bits, float p, float inv_keep) {
    const uint32_t thresh = (uint32_t)ceilf(p * 16777216.0f);
    return (bits >> 8) >= thresh ? inv_keep : 0.f;
}

template <int W> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <int W> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
// sum of up to 1024 values, one per thread (deterministic: wave butterflies, then 16 wave sums in order)
__device__ __forceinline__ float block_sum_1024(float v, float* s16) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s16[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += s16[w];
    return t;
}

// ---- reductions over the LPH lanes of one head group.  DPP row operations (one VALU op each) instead of
// ds_bpermute: row_half_mirror pairs lane i with 7-i inside each 8 lanes, quad_perm covers xor 1 / xor 2.
// (mov_dpp with bound_ctrl: no `old` operand to materialise -- every lane of these permutations has a source -- so the compiler folds
// the move into the add that consumes it: one v_add_f32_dpp per reduction step instead of zero + v_mov_b32_dpp + add)
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int kDppXor1 = 0xB1;        // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;        // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141; // lane i <- lane 7-i  (within 8)
constexpr int kDppMirror = 0x140;     // lane i <- lane 15-i (within 16)

template <int W> __device__ __forceinline__ float head_sum(float v) {
    static_assert(W == 4 || W == 8 || W == 16 || W == 32, "head group width");
    if (W == 32) v += __shfl_xor(v, 16);
    if (W >= 16) v += dpp_mov<kDppMirror>(v);
    if (W >= 8) v += dpp_mov<kDppHalfMirror>(v);
    v += dpp_mov<kDppXor2>(v);
    v += dpp_mov<kDppXor1>(v);
    return v;
}
template <int W> __device__ __forceinline__ float head_max(float v) {
    if (W == 32) v = fmaxf(v, __shfl_xor(v, 16));
    if (W >= 16) v = fmaxf(v, dpp_mov<kDppMirror>(v));
    if (W >= 8) v = fmaxf(v, dpp_mov<kDppHalfMirror>(v));
    v = fmaxf(v, dpp_mov<kDppXor2>(v));
    v = fmaxf(v, dpp_mov<kDppXor1>(v));
    return v;
}


struct __attribute__((packed, aligned(4))) i32x2u { int x, y; };       // 4-byte aligned pairs: one dwordx2 load
struct __attribute__((packed, aligned(4))) f32x2u { float x, y; };
struct __attribute__((packed, aligned(4))) f32x4u { float x, y, z, w; };
__device__ __forceinline__ i32x2u ldp(const int32_t* p) { return *reinterpret_cast<const i32x2u*>(p); }
__device__ __forceinline__ f32x2u ldp(const float* p) { return *reinterpret_cast<const f32x2u*>(p); }
__device__ __forceinline__ void stp(float* p, float a, float b) { f32x2u v; v.x = a; v.y = b; *reinterpret_cast<f32x2u*>(p) = v; }


__device__ __forceinline__ float4 ld4_off(const float* base, uint32_t byte_off) {      // scalar base + 32-bit offset
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ float ld1_off(const float* base, uint32_t byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
// the same for stores: a wave-uniform base pointer + a 32-bit byte offset is ONE address register per lane (global_store ... saddr);
// `p + (size_t)row * 128 + lane * 4` is a 64-bit multiply-add per lane and store (v_lshl_add_u64: 72 of the 672 vector instructions
// of the forward attention loop in round 4)
__device__ __forceinline__ void st4_off(float* base, uint32_t byte_off, float4 v) {
    *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + byte_off) = v;
}
__device__ __forceinline__ void st1_off(float* base, uint32_t byte_off, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
}
// ---- store policy of the row tables (DESIGN.md §3 classifies every table of the training step by its next reader;
// profiles/store_policy_probe.txt is the measurement).  A table is written through a wave-uniform base + a 32-bit byte offset, as with
// st4_off / st1_off, because the flavours below exist only as buffer stores the compiler itself tracks (it counts vmcnt; no inline
// assembly): the base becomes an unbounded raw-buffer descriptor in four SGPRs, the offset is the one address register.
//   st4_next / st1_next : tables the NEXT launch reads -- write-through (sc1): the line is not left dirty in the XCD's L2 for the
//                         kernel boundary to write back (boundary 3.1-4.2 -> 1.3-1.6 us behind 16-64 MB), and the memory-side cache still
//                         holds it for the consumer (a consumer's pass: 9.6 us of 64 MB either way; behind nt stores 23.8 us)
//   st4_late / st1_late : tables only the backward pass reads, hundreds of microseconds later -- write-through and non-temporal
//                         (nt sc1): the same boundary, and the follower's own reads are not pushed out of the memory-side cache
// The 4-byte twins (the [n, H] and per-edge tables) take their class's flavour only under -DFN_STORE_POLICY=2: the probe measured 16-byte
// stores, and a write-through store is one fabric write whatever its width, so until a 4-byte arm is measured they stay plain.
// -DFN_STORE_POLICY=0: every one of them is the plain st4_off / st1_off (the A/B arm; same values either way, only the cache policy differs)
#ifndef FN_STORE_POLICY
#define FN_STORE_POLICY 1
#endif
constexpr int kStNext = 16, kStLate = 18;      // cache-policy bits of a gfx950 buffer store: 1 sc0, 2 nt, 16 sc1
template <int AUX> __device__ __forceinline__ void st4_policy(float* base, uint32_t byte_off, float4 v) {
#if FN_STORE_POLICY && defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned u32x4 __attribute__((__vector_size__(16)));
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const f32x4_t w = {v.x, v.y, v.z, v.w};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, w), __builtin_amdgcn_make_buffer_rsrc(base, 0, -1, 0x00020000), (int)byte_off, 0, AUX);
#else
    st4_off(base, byte_off, v);
#endif
}
template <int AUX> __device__ __forceinline__ void st1_policy(float* base, uint32_t byte_off, float v) {
#if FN_STORE_POLICY >= 2 && defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), __builtin_amdgcn_make_buffer_rsrc(base, 0, -1, 0x00020000), (int)byte_off, 0, AUX);
#else
    st1_off(base, byte_off, v);
#endif
}
__device__ __forceinline__ void st4_next(float* base, uint32_t byte_off, float4 v) { st4_policy<kStNext>(base, byte_off, v); }
__device__ __forceinline__ void st4_late(float* base, uint32_t byte_off, float4 v) { st4_policy<kStLate>(base, byte_off, v); }
__device__ __forceinline__ void st1_next(float* base, uint32_t byte_off, float v) { st1_policy<kStNext>(base, byte_off, v); }
__device__ __forceinline__ void st1_late(float* base, uint32_t byte_off, float v) { st1_policy<kStLate>(base, byte_off, v); }



// ---- explicit address spaces.  Pointers read out of an argument block in memory are generic; dereferenced as such they become
// flat_load / flat_store, which tick BOTH wait counters and so serialise with the LDS traffic.  Hot accesses cast to the global
// (G()) or LDS address space.
typedef float f32x4 __attribute__((ext_vector_type(4)));       // MFMA accumulator / 16-byte vector
#define DN_MFMA(ACC, AV, BV) ACC = __builtin_amdgcn_mfma_f32_16x16x4f32(AV, BV, ACC, 0, 0, 0)      // dense_head.inc, wgrad128.inc
#define FN_LDS __attribute__((address_space(3)))
#define FN_GLB __attribute__((address_space(1)))
typedef FN_LDS float lds_f;
typedef FN_LDS int lds_i;
typedef FN_GLB float glb_f;
typedef FN_GLB int glb_i;
__device__ __forceinline__ const glb_f* G(const float* p) { return (const glb_f*)p; }
__device__ __forceinline__ glb_f* G(float* p) { return (glb_f*)p; }
__device__ __forceinline__ const glb_i* G(const int* p) { return (const glb_i*)p; }
__device__ __forceinline__ float4 ld4(const glb_f* p) {
    const f32x4 v = *reinterpret_cast<const FN_GLB f32x4*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(glb_f* p, float4 v) { *reinterpret_cast<FN_GLB f32x4*>(p) = (f32x4){v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 ld4s(const lds_f* p) {
    const f32x4 v = *reinterpret_cast<const FN_LDS f32x4*>(p);
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4s(lds_f* p, float4 v) { *reinterpret_cast<FN_LDS f32x4*>(p) = (f32x4){v.x, v.y, v.z, v.w}; }

// LDS-DMA (global_load_lds_*): the wave's 64 lanes write 64 x SIZE consecutive bytes at the wave-uniform LDS address; the
// global source address is per lane.  No VGPR destination: the tile costs no registers while it is in flight.
template <int SIZE>
__device__ __forceinline__ void dma_to_lds(const void* gsrc, void* lds_wave_base) {
    static_assert(SIZE == 4 || SIZE == 16, "dword or dwordx4 pieces");
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (SIZE == 16) __builtin_amdgcn_global_load_lds((const FN_GLB void*)gsrc, (FN_LDS void*)lds_wave_base, 16, 0, 0);
    else __builtin_amdgcn_global_load_lds((const FN_GLB void*)gsrc, (FN_LDS void*)lds_wave_base, 4, 0, 0);
#endif
}

}  // namespace
