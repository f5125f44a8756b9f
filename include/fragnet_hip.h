/*
 * libfragnet_hip.so -- C-ABI of the MI355X (gfx950) kernels behind FragNet's message-passing hot path.
 *
 * This is the drop-in boundary of SURVEY.md §8(b): everything the reference obtains from the
 * un-vendored torch-scatter / torch_geometric wheels on this path, plus the fused per-level
 * kernels that replace the reference's index_select/cat/mul/sum/scatter chains.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes; no torch types.
 *   - every pointer is a DEVICE pointer into caller-owned memory; the library never allocates,
 *     frees or retains pointers; workspaces are caller-provided.
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no
 *     internal synchronisation, no default-stream use; stateless and re-entrant -- with two documented
 *     exceptions that are process-wide settings, meant to be set once before the first compute call and not
 *     changed while another thread is inside the library: the tuning table (fn_set_tuning) and the profiling
 *     stamp buffer (fn_debug_set_stamps).  Kernels never read either; only launch decisions on the host do.
 *   - return 0 on success, a negative FN_E* code for an argument error, or a positive
 *     hipError_t taken right after the launch.  fn_last_error() describes the last failure
 *     on the calling thread.
 *   - float data is fp32, row-major, feature width D = 128 (= heads * head_dim) where stated;
 *     index data is int32 in plans (int64 only where the batch dict hands it over).
 *
 * Reference call sites each entry point replaces are cited as file:line under
 * /root/reference/fragnet/.
 */
#ifndef FRAGNET_HIP_H
#define FRAGNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FN_ABI_VERSION 12
#define FN_D 128              /* feature width of every node table on the path (emb_dim) */
#define FN_MAX_TASKS 16       /* CSR builds fused into one fn_plan_build call */
#define FN_MAX_EDGE_K 8       /* widest raw edge attribute folded in-kernel (6 for fragment bonds) */

#define FN_EINVAL (-1)        /* null pointer / negative size / misaligned */
#define FN_EUNSUPPORTED (-2)  /* heads or width not in {1,2,4,8} x 128 */
#define FN_ETOOMANY (-3)      /* more than FN_MAX_TASKS tasks */

typedef void* fn_stream_t;    /* hipStream_t */

int fn_abi_version(void);

/* Process-wide tuning knobs (defaults are the measured best for MI355X; the bench uses them for A/B runs).
 * FN_TUNE_FWD_BLOCKS: workgroups of the attention kernels that are resident at once in a TRAINING pass (forward with the
 *   dropout epilogue, source pass of the backward): default 1024 = 256 CUs x 4 (768 until round 5's re-sweep of the launch
 *   shapes, profiles/r05_launch_shape_sweep.txt); a level with more row groups than that gives
 *   every half-wave several consecutive rows to software-pipeline (4 at ESOL batch 512).  FN_TUNE_FWD_BLOCKS_EVAL (1792 =
 *   256 x 7) is the same for the plain forward (inference, or training without dropout).
 * fn_set_tuning refuses (FN_EINVAL, table untouched) a value outside a key's range, stated in [] below; retired keys take anything.
 *   FN_TUNE_FWD_BLOCKS [1, 2^20]; FN_TUNE_FWD_BLOCKS_EVAL [1, 2^20]. */
#define FN_TUNE_FWD_BLOCKS 0
#define FN_TUNE_GEMM_SLOTS 1   /* > 0: cap on the workgroups of a projection GEMM launch (1024 = 256 CUs x 4 resident); a launch with
                                * more 64x64 output tiles then walks several row tiles per workgroup, prefetching the next tile's
                                * rows.  Default 0 = one tile per workgroup (faster at every measured size).  [0, 2^20] */
#define FN_TUNE_RETIRED_2 2     /* (retired in round 3, no effect: parameter-gradient work and the fragment-bond chain forked onto side streams --
                                * a forked hipGraph replays SLOWER than the serial one on ROCm 7.2, 1.84 vs 1.69 ms per step) */
#define FN_TUNE_WGRAD_BLOCKS 3 /* target workgroup count of the grouped weight-gradient launch of a backward pass (default 192 since round 5's re-sweep -- with layer 0's workgroups the launch then has 1.6 per CU; 256: + 1 % per step; 512 wrote twice the partials).  [1, 2^20] */
#define FN_TUNE_RETIRED_4 4     /* (retired in round 3, no effect: the molecule-resident fused FORWARD of round 2 -- measured equal at 512
                                * molecules, slower elsewhere; source kept out of the build under tools/probe/retired/mol_fused.inc) */
#define FN_TUNE_RETIRED_5 5     /* (retired: phase skew of that kernel) */
#define FN_TUNE_RETIRED_6 6     /* (retired: register-resident-weights projection kernel k_proj128, 1-4 % slower per step) */
#define FN_TUNE_FUSE_ROWDOTS 7 /* 1 (default): inside fn_encoder_forward the bond-graph attention kernel also writes the atom graph's edge
                                * term <new_bond, a[:, d:d+128]> from the row it holds in registers; 0: a separate row-dots launch.  [0, 1] */
#define FN_TUNE_WGRAD_DIRECT 8 /* 1 (default): the grouped K = 128 weight-gradient partials run as k_wgrad128_multi (operands straight from
                                * global memory in the MFMA layout, csrc/wgrad128.inc); 0: the LDS-staged k_linear128_wgrad_multi (also
                                * what layer 0's narrow products use).  [0, 1] */
#define FN_TUNE_RETIRED_9 9     /* (retired: wave-independent projection kernel k_proj_direct, 1 % slower per step) */
#define FN_TUNE_FWD_BLOCKS_EVAL 10
#define FN_TUNE_DST_BLOCKS 11  /* target workgroup count of the backward destination pass (default 1536: three rows per half-wave at ESOL batch
                                * 512; never more than three rows, see prep_gat_bwd_dst).  [1, FN_MAX_PART] */
#define FN_TUNE_SRC_BLOCKS 12  /* resident workgroups of the backward source pass (default 512; every block writes a row of partial sums).  [1, 1024] */
#define FN_TUNE_RD_BLOCKS 13   /* (default 512; 256 until round 5) workgroups of the edge-term backward that shares the source pass's launch (each writes a row of partial sums; a table holds FN_MAX_PART rows).  [1, FN_MAX_PART] */
#define FN_TUNE_GEMM_COLAUNCH 14 /* inside fn_encoder_*: the 128 -> 128 projections (forward) and input-gradient products (backward) that do
                                 * not depend on an attention pass ride along as extra workgroups of that pass's launch (the atom projection
                                 * beside the bond + fragment-bond levels, the next layer's bond / fragment-bond projections beside the atom
                                 * level; mirrored in the backward), layer 0's three raw-feature projections share a launch and all weight-gradient
                                 * partial products of a backward pass are one launch.  != 0 (default 2): on, the GEMM workgroups first in the
                                 * launch (after / interleaved with the attention workgroups measured slower and were removed in round 3:
                                 * profiles/r02e_colaunch_ab.txt); 0: separate launches.  [0, 2] */
#define FN_TUNE_RETIRED_15 15    /* (retired: persistent riding GEMM workgroups walking several tiles, slower) */
#define FN_TUNE_RETIRED_16 16    /* (retired: raised wave priority of the riding workgroups, no effect) */
#define FN_TUNE_RETIRED_17 17    /* (retired in round 5: the two-pass backward's atom chain beside the bond chain -- superseded by the one-pass
                                  * backward; the two passes remain as the general path, in plain dependency order) */
#define FN_TUNE_RETIRED_18 18    /* (retired in round 5: the molecule-resident single-pass backward of round 3 -- 39 us against 28 for a level;
                                  * source kept out of the build under tools/probe/retired/mol_bwd.hip) */
#define FN_TUNE_RETIRED_19 19    /* (retired: test hook of that kernel) */
#define FN_TUNE_MOL_TAIL 20           /* 1 (default): batches marked molecule-contiguous (fn_encoder.mol_contiguous) run the last layer's
                                       * fragment tail -- fragment sums, fragment graph, readout and their backward -- as one
                                       * molecule-resident launch each way (csrc/mol_tail.inc); 0: the separate launches;
                                       * 2 (test hook): fused, every molecule on the global-memory path of oversize molecules.  [0, 2] */
#define FN_TUNE_WGRAD0_ROWS 21        /* layer 0's weight-gradient products (K = 167 / 17 / 6): rows per block as a multiple of the
                                       * per-product rule (M / 256 rounded up to 32); tens digit = the product with K > 128 (atoms),
                                       * units digit = the narrow ones (a digit 0 counts as 1).  Default 23.  [1, 99] */
#define FN_TUNE_BWD_ONE 22            /* 1: fn_encoder_backward runs every attention level's backward (bond / atom / fragment-bond graph) as
                                       * ONE source-owner pass (csrc/gat_bwd_one.inc): the forward then also writes out2 / sigma and the
                                       * producers of the gradient rows write the node-local dots c, g_s_dst; 0: the two-pass backward.  [0, 1] */
#define FN_TUNE_ONE_BLOCKS 23         /* target workgroups per LEVEL of a one-pass backward launch (default 768 = five rows per half-wave at the bond level of ESOL batch 512; every block writes a row of
                                       * partial sums, so at most FN_MAX_PART).  Round 5's re-sweep: 1024 + 1.0 %, 512-896 within noise, 384 and fewer slower.  [1, FN_MAX_PART] */
#define FN_TUNE_PAD_SKIP 24           /* 1 (default): with the one-pass backward on a molecule-contiguous static-shape batch the kernels skip the
                                       * padding rows (zero rows out, no gathers, no GEMM tiles, no weight-gradient rows); 0: they are processed.  [0, 1] */
#define FN_TUNE_ONE_INTERLEAVE 25      /* 1: in the one-pass backward's three-level launch the bond level's workgroups alternate with the atom /
                                       * fragment-bond levels'; 0 (default): level after level (alternating measured 42-46 us against 37-40).  [0, 1] */
#define FN_TUNE_ONE_TIER6 26           /* 1 (default): the attention kernels' gather tiers include 6 rows (forward 4 / 6 / 8, one-pass backward
                                       * 4 / 6 / 8 / 12 per round trip); 0: 4 / 8 (/ 12).  [0, 1] */
#define FN_TUNE_RIDER_PIECES 27       /* 16-byte pieces per thread of the Adam slice that rides in the deferred-reduction launch (fn_encoder.adam_rider):
                                       * 1 (default) = as many 1024-thread workgroups as the slice has KiB x 16.  [1, 4096] */
#define FN_TUNE_RIDER_AT 28           /* which launch of the one-pass encoder backward carries fn_encoder.adam_rider: 0 (default) the last one (the
                                       * deferred reductions: + 7 us there for the 12.9 - 4.5 us the step's Adam launch saves), 1 the first one (the
                                       * molecule-resident fragment tail, when it runs: + 11.7 us).  [0, 1] */
#define FN_TUNE_RETIRED_29 29          /* (retired, no effect: the DEFERRED forms of the engine's one-pass backward, four heads.  1: the forward wrote no
                                       * out2 / sigma, the pass left dz at the edges' destination-order slots and the consumers of g_h added the
                                       * g_s_dst a_dst term -- one more MFMA step in the input-gradient products, the weight-gradient kernels' side
                                       * product U = G^T X for dL/da_dst, k_gsd_seg for layer 0; 2: the mixed form, layers >= 1 deferred and layer 0
                                       * plain.  Both measured slower than the default at ESOL batch 512: 0.797 against 0.783 ms per step for the
                                       * all-layer form (round 5), 0.782 against 0.764 ms for the mixed form (round 6,
                                       * profiles/r06_mixed_deferred_form_ab.txt).  Last commit that contains it: 38e95ae.  The stand-alone operator
                                       * keeps its deferred form: fn_gat_bwd_one_f32 with dz_em, fn_gat_gsd_f32) */
#define FN_TUNE_FWD_BLOCKS_EVAL_LARGE 30 /* the plain forward (inference) of a level with more than 4 x FN_TUNE_FWD_BLOCKS_EVAL row groups (2048+ molecules
                                       * per batch) runs this many workgroups instead (default 6144): with the fixed count every half-wave walked 12-46
                                       * rows and the launch waited for its slowest workgroups.  0: one count for every size (rounds 1-4).  [0, 2^20] */
#define FN_TUNE_FWD_TAIL_ROWS 31       /* > 0: in the two-level forward launch (bond + fragment-bond graph) the SECOND level's half-waves take at most this
                                       * many rows: its workgroups are dispatched last, so long-lived ones are the launch's tail (only large batches
                                       * reach the cap: 2048 molecules per batch forward-only 1.13 -> 1.28 M molecules/s).  Evaluation passes only (no dropout
                                       * epilogue), as FN_TUNE_FWD_BLOCKS_EVAL_LARGE.  Default 1; 0: no cap.  [0, 2^20] */
#define FN_TUNE_DENSE_TILES 32         /* 1 (default): fn_dense_fwd_f32 runs inputs of >= 192 tiles of 64 x 128 (1536+ rows at N = 1024) with K a multiple of 32 on
                                       * workgroup-shared LDS macro-tiles (k_dense_fwd_tiles, round 6: 62 -> 43 us at M = 2048, K = N = 1024); 0: the per-wave
                                       * operand kernel for every shape (A/B, and the parity test of the two against each other).  [0, 1] */
#define FN_TUNE_ENGINE_CONST 33        /* 1 (default): the attention launches of the engine (four heads, levels of >= 2 edges, no probs_orig / stamp buffer)
                                       * run kernel instances in which their uniform run-time flags are compile-time constants -- a training pass:
                                       * edge-major probabilities, relu(dropout(.)) epilogues with p > 0 (forward kind 2, the one-pass backward's EN
                                       * instances); an evaluation pass: head-major probabilities, ReLU epilogues without dropout (forward kind 3).  Same
                                       * arithmetic, bit-identical results, fewer scalar tests and branches in the issue-bound row loops (round 6: 0.769 ->
                                       * 0.755 ms per training step, the forward-only sweep - 4 ... - 7 %); 0: the general instances for every launch (A/B,
                                       * and the parity test of the two against each other).  [0, 1] */
#define FN_TUNE_COALITION_STAGED 34     /* the form of fn_pool_cat_coalitions_f32's kernel.  0: one workgroup per output row and half, the form of
                                       * fn_pool_cat_groups_f32.  n >= 2: the tiled form -- a workgroup owns 64 consecutive output rows and walks the runs
                                       * of one molecule in them; a run of at least n - 1 rows is staged (the molecule's atom rows go to LDS once for all
                                       * of its rows), a shorter one reads global memory (2: every run is staged; a large n: none).  1 (default): the
                                       * tiled form with n = 17 for a call with at least 64 rows per molecule on average, where it measured faster,
                                       * else the form of 0.  Same bits in every form.  [0, INT_MAX] */
#define FN_TUNE_COUNT 35
/* The table at load, in key order (fn_get_tuning reads it back):
 *   1024, 0, 0, 192, 0, 0, 0, 1, 1, 0, 1792, 1536, 512, 512, 2, -1, 0, 1, 0, 0, 1, 23, 1, 768, 1, 0, 1, 1, 0, 0, 6144, 1, 1, 1, 1 */
int fn_set_tuning(int key, int value);
/* The current value of a key; 0 for a key outside the table.  Added under ABI 12 (nothing existing changes). */
int fn_get_tuning(int key);
/* Profiling aid (process-wide, like the tuning knobs): while `buf` (device, n_u64 >= 16 * 4 * workgroups 64-bit words) is set, every wave
 * of the one-pass attention backward (fn_gat_bwd_one_f32) writes s_memtime stamps of its phases into it (tools/probe/bwd_one_probe.py
 * --stamps).  NULL switches it off (the default: the kernel then pays one uniform branch per phase). */
int fn_debug_set_stamps(void* buf, int64_t n_u64);
/* Profiling aid (process-wide; ABI 12): four hipEvent_t (created with timing enabled) or NULL entries -- events[0] / [1] are recorded
 * right before / behind the bond-graph level's forward launch of layer 0 in fn_encoder_forward (k_gat_fwd_pair: bond + fragment-bond
 * levels), events[2] / [3] around the same level's one-pass backward launch in fn_encoder_backward (k_gat_bwd_one3 of layer 0).
 * On a capturing stream they become EXTERNAL event-record nodes (hipEventRecordExternal), so hipEventElapsedTime between a pair
 * after a replay is that launch's duration INSIDE the captured step -- what bench.py's `roofline` quotes.  NULL (the default, also
 * `events` == NULL) records nothing.  The events stay the caller's. */
int fn_debug_set_profile_events(void* const* events);
const char* fn_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Graph plan: destination-sorted CSRs, built once per batch and reused by all layers, fwd+bwd.
 * Replaces the implicit index handling inside torch_scatter.scatter_add / scatter_softmax
 * (model/gat/gat2.py:153,162,210,216,234,257,265,303,309,820,821) and
 * torch_geometric.utils.add_self_loops (gat2.py:179: `n_loops` identity items i -> segment i
 * appended after the real ones).
 *
 * One call builds up to FN_MAX_TASKS CSRs over a concatenated segment space:
 *   rowptr_all[seg_base + s]            global position of segment s's first item
 *   perm_all  [item_base + p]           task-local item id at sorted position p, ascending inside
 *                                       a segment (=> deterministic, reference summation order)
 * For a GAT level, two tasks are paired (role DST keyed by destination, role SRC keyed by source):
 *   DST task: aux_a[pos] = source node of the edge at pos; aux_b[item] = position of edge `item` (inverse perm)
 *             aux_c[pos] = position of the same edge in the paired SRC task
 *   SRC task: aux_a[pos] = destination node; aux_b[pos] = that edge's position (task-local) in the
 *             paired DST task
 * ------------------------------------------------------------------------------------------ */
#define FN_ROLE_PLAIN 0
#define FN_ROLE_DST 1
#define FN_ROLE_SRC 2

typedef struct fn_csr_task {
    const int64_t* key;        /* [n_real] segment id per item (device)                        */
    const int64_t* other_key;  /* [n_real] the opposite endpoint (roles DST/SRC), else NULL     */
    int64_t n_real;            /* items with an explicit key                                    */
    int64_t n_loops;           /* identity items appended: item n_real+i belongs to segment i   */
    int64_t n_seg;             /* number of segments                                            */
    int64_t item_base;         /* filled by fn_plan_layout                                      */
    int64_t seg_base;          /* filled by fn_plan_layout                                      */
    int32_t role;              /* FN_ROLE_*                                                     */
    int32_t partner;           /* index of the paired task (roles DST/SRC), else -1             */
} fn_csr_task;

/* Host-side helper: fills item_base/seg_base, returns totals. */
int fn_plan_layout(fn_csr_task* tasks, int n_tasks, int64_t* total_items, int64_t* total_segs);

/* ws_i32 must hold FN_PLAN_WS(total_segs, total_items) int32.  ws_i32[total_segs + total_items] is a
 * status word: non-zero after the call completes if any key was outside [0, n_seg). */
#define FN_PLAN_WS(total_segs, total_items) ((total_segs) + 2 * (total_items) + 4 + 2 * ((total_segs) / 2048 + 1) + 2)
#define FN_PLAN_WS_ZEROED(total_segs, total_items) ((total_segs) + (total_items) + 4 + 2 * ((total_segs) / 2048 + 1) + 2)   /* the leading part that must be zero (FN_PLAN_PREZEROED) */
int fn_plan_build(const fn_csr_task* tasks, int n_tasks,
                  int32_t* rowptr_all /*[total_segs+1]*/, int32_t* perm_all /*[total_items]*/,
                  int32_t* aux_a /*[total_items]*/, int32_t* aux_b /*[total_items]*/, int32_t* aux_c /*[total_items]*/,
                  int32_t* ws_i32, int32_t flags /*FN_PLAN_**/, fn_stream_t stream);

/* The same plan for a MOLECULE-CONTIGUOUS batch in one launch (csrc/mol_plan.hip).  collate_fn concatenates molecules
 * (dataset/data.py:877-948): every index space (atoms, directed bonds, bond-graph edges, fragments, fragment connections,
 * fragment-bond-graph edges, molecules, ...) is a concatenation of per-molecule ranges and every key of molecule i is smaller
 * than every key of molecule i + 1, so the stable sort of each CSR is the concatenation of per-molecule sorts: one workgroup per
 * molecule sorts in LDS.  `offsets` (device, int32 [n_spaces][n_mols + 1]) = first index of molecule i in each space (the
 * collate's cumulative counts); node_space / item_space name, per task, the spaces its segments and its items live in.
 * Static-shape batches (fn_stage_padded): counts_dev = number of real molecules, offsets rows beyond it repeat the real
 * totals, cap = array lengths, pad_mod = reserved slots per space; the padding tail (item c of a field pointing into space s
 * holds cap[s] - 1 - (c - n_real) % pad_mod[s]) is written in closed form.  max_per_mol: upper bound of a molecule's extent in
 * each space (sizes the LDS tile: <= 64 KB in total, else FN_EUNSUPPORTED); a larger molecule sets status bit 2 (value 4), a key
 * outside its molecule's node range bit 1 (value 2).  pad_hint: upper bound of the padding items per space (grid sizing; 0: none).
 * Same outputs, bit for bit, as fn_plan_build; ws_i32 only carries the status word (same place). */
#define FN_MAX_SPACES 8
typedef struct fn_mol_layout {
    const int32_t* offsets;
    int32_t n_spaces, pad_;
    int64_t n_mols;
    int32_t node_space[FN_MAX_TASKS], item_space[FN_MAX_TASKS];
    const int32_t* counts_dev;             /* nullable */
    int64_t cap[FN_MAX_SPACES], pad_mod[FN_MAX_SPACES], max_per_mol[FN_MAX_SPACES], pad_hint[FN_MAX_SPACES];
} fn_mol_layout;
int fn_plan_build_mol(const fn_csr_task* tasks, int n_tasks, const fn_mol_layout* layout, int32_t* rowptr_all, int32_t* perm_all,
                      int32_t* aux_a, int32_t* aux_b, int32_t* aux_c, int32_t* ws_i32, int32_t flags, fn_stream_t stream);
/* flags: the caller has already zeroed rowptr_all[0 .. total_segs] and the whole of ws_i32 on this stream (a captured step
 * lets the staging launch in front of the replay do it, FN_STAGE_ZERO): fn_plan_build skips its zeroing launch */
#define FN_PLAN_PREZEROED 1

/* ------------------------------------------------------------------------------------------
 * One attention level (bond graph, atom graph, fragment-bond graph, fragment graph):
 *   z_e = s_dst[dst] + s_src[src] + s_edge[e];  l_e = LeakyReLU(z_e);  p = softmax over in-edges
 *   out[dst] = sum_e p_e * h[src]
 * Replaces, per level, index_select x3 + cat + mul + sum + LeakyReLU + scatter_softmax + mul +
 * scatter_add at gat2.py:146-164, 196-218, 250-267, 286-311.
 *
 * `att` is the reference's attention parameter [heads, att_w] = [dst | edge | src] blocks
 * (a_b / f_a_b: att_w = 3d; a / f: att_w = 2d + 128).
 * ------------------------------------------------------------------------------------------ */

/* s_dst[n,H] = <h[n,head,:], att[head, dst_off:+d]>, s_src likewise (gat2.py:150,208,254,300). */
int fn_node_scalars_f32(const float* h /*[n,128]*/, const float* att, int att_w, int dst_off, int src_off,
                        float* s_dst /*[n,H]*/, float* s_src /*[n,H]*/, int64_t n, int heads, fn_stream_t stream);

/* Edge term of the logit, always addressed by DESTINATION-SORTED edge position (coalesced, no
 * dependent gather).  All per-edge arrays of a level are HEAD-MAJOR ([H][m], [K][m]): the two consecutive
 * in-edges a lane owns are then one 8-byte load.
 * mode 0: s_sorted [H,m] given (fn_row_dots_sorted_f32; 0 at loop positions).
 * mode 2: s[pos,h] = <embW x_sorted[pos] + embb, att[h, mid_off:+d_e]> folded in-kernel (the reference's
 * edge_attr_bond_embed / edge_attr_fbond_embed Linear(K -> d_e), gat2.py:139,242); x_sorted is the raw
 * attribute permuted once per batch by fn_sort_edge_attr_f32 (it is the same in every layer).  A loop item's raw attribute is
 * zero (x_sorted is 0 at loop positions), so its term is <embb, att[h, mid_off:+d_e]> -- the reference adds self loops to the atom
 * graph only, which is mode 0 (a zero row there: term 0). */
typedef struct fn_edge_term {
    int32_t mode;
    int32_t K;                /* mode 2: raw attribute width (1 or 6) */
    int32_t d_e;              /* mode 2: embed width (= head_dim)     */
    int32_t mid_off;          /* mode 2: offset of the edge block in att */
    const float* s_sorted;    /* mode 0: [H, m] */
    const float* x_sorted;    /* mode 2: [K, m] */
    const float* embW;        /* mode 2: [d_e, K]    */
    const float* embb;        /* mode 2: [d_e]       */
    const float* x_src;       /* mode 2, nullable, read by fn_gat_bwd_one_f32 only: [K, m] the raw attribute in SOURCE order
                               * (fn_sort_edge_attr_src_f32); NULL: that pass gathers it from x_sorted */
} fn_edge_term;

typedef struct fn_gat_plan {          /* slices of the fn_plan_build outputs for one level */
    const int32_t* rowptr_d;  /* [n+1] global positions (DST task)  */
    const int32_t* eid_d;     /* [m]   original edge id at sorted pos */
    const int32_t* src_d;     /* [m]   source node at sorted pos      */
    const int32_t* rowptr_s;  /* [n+1] (SRC task)                     */
    const int32_t* dst_s;     /* [m]   destination node               */
    const int32_t* dpos_s;    /* [m]   position in the DST order      */
    const int32_t* inv_d;     /* [m]   original edge id -> position in the DST order */
    const int32_t* spos_d;    /* [m]   DST position -> position in the SRC order     */
    int32_t pos_base_d;       /* item_base of the DST task            */
    int32_t pos_base_s;       /* item_base of the SRC task            */
    int64_t n;                /* nodes                                */
    int64_t m;                /* edges incl. loop items               */
    int64_t m_real;           /* edges with an explicit attribute     */
} fn_gat_plan;

/* a plain CSR of fn_plan_build (segment sums, pooling, molecule membership) */
typedef struct fn_seg_plan {
    const int32_t* rowptr;    /* [n_seg+1] global positions */
    const int32_t* perm;      /* [n_items] */
    const int64_t* index;     /* [n_items] the original key (for the gather backward) */
    int64_t n_seg, n_items;
    int32_t pos_base, pad_;
} fn_seg_plan;

/* Optional fused epilogue of the forward kernel: y = relu?(dropout(out)) with the Philox stream of
 * fn_dropout_act_f32 (block index = element / 4), so the standalone backward kernel applies to it. */
typedef struct fn_act_epilogue {
    float* y;                 /* [n,128]; NULL = no fused activation */
    float p;                  /* dropout probability (0 = none)      */
    int32_t relu;
    uint64_t seed, offset;
    const uint64_t* offset_dev; /* nullable: a device-resident counter ADDED to offset when the kernel runs, so that a
                                 * captured hipGraph draws fresh masks on every replay (the owner advances it in-graph) */
} fn_act_epilogue;

/* p_sorted [H,m] (head-major): probabilities in destination-sorted order; the sign bit carries "z_e <= 0"
 * (the LeakyReLU branch) for the backward pass.  probs_orig (nullable) [m,H] in original edge
 * order, unsigned -- the reference's attn_probs. */
int fn_gat_fwd_f32(const float* h, const float* s_dst, const float* s_src, const float* att, int att_w,
                   const fn_edge_term* et, const fn_gat_plan* plan, float neg_slope,
                   float* out /*[n,128], nullable when act->y is given*/, float* p_sorted /*[H,m]*/,
                   float* probs_orig /*nullable*/,
                   float* out2 /*nullable: [n,128] = sum_e lambda_e p_e h[src_e], lambda_e = 1 (z_e > 0) or neg_slope*/,
                   float* sigma /*with out2: [n,H] = sum_e lambda_e p_e -- what fn_gat_bwd_one_f32's caller needs*/,
                   int p_edge_major /*1: p_sorted is written [m,H] (one cache line per edge, for fn_gat_bwd_one_f32) instead of [H,m]*/,
                   const fn_act_epilogue* act /*nullable*/, int heads, fn_stream_t stream);

/* Backward, destination pass.  Writes, per edge, (|p|, dz) into pz_src [H,m,2] at the edge's slot in SOURCE
 * order (so the source pass streams them), dz_sorted [H,m] in mode 0 (= dL/ds_sorted, the gradient of the edge
 * term), g_s_dst [n,H]; mode 2 writes per-block partial sums part_e [grid, H*(K+1)].
 * Returns the grid size used through *n_part_e. */
int fn_gat_bwd_dst_f32(const float* g_out, const float* h, const float* p_sorted, const fn_edge_term* et,
                       const fn_gat_plan* plan, float neg_slope,
                       float* dz_sorted /*mode 0, nullable: [H,m] destination-sorted (autograd path)*/,
                       float* g_s_orig /*mode 0, nullable: [m_real,H] original edge order (engine path)*/,
                       float* pz_src, float* g_s_dst,
                       float* part_e /*mode2: [FN_MAX_PART, H*(K+1)]*/, int* n_part_e,
                       int heads, fn_stream_t stream);

/* Backward, source pass: g_h [n,128] = sum_{e: src=n} p_e g_out[dst] + g_s_dst*a_dst + g_s_src*a_src,
 * and per-block partial sums of dL/da_dst, dL/da_src: part_a (column-major [256][FN_MAX_PART]). */
int fn_gat_bwd_src_f32(const float* g_out, const float* h, const float* pz_src,
                       const float* g_s_dst, const float* att, int att_w, int dst_off, int src_off,
                       const fn_gat_plan* plan, float* g_h, float* part_a, int* n_part_a,
                       int heads, fn_stream_t stream);

/* Backward of one attention level as ONE source-owner pass (csrc/gat_bwd_one.inc; the autograd of gat2.py:146-169, 196-219,
 * 250-268, 286-312).  Replaces fn_gat_bwd_dst_f32 + fn_gat_bwd_src_f32 when the caller supplies the two node-local dots
 *     cdot[t,h]    = <g_out[t,h,:], out[t,h,:]>                          (= sum_e p_e <g_out[t], h[src_e]>, since out = sum_e p_e h[src_e])
 *     g_s_dst[t,h] = <g_out[t,h,:], out2[t,h,:]> - cdot[t,h] sigma[t,h]  (= sum_{e -> t} dz_e)
 * (fn_gat_cu_f32, or the epilogue of the input-gradient GEMM inside fn_encoder_backward).  Outputs as the two passes': g_h
 * [n,128]; mode 0: dz_sorted [H,m] (destination order) and / or g_s_orig [m_real,H] (original edge order), both nullable;
 * mode 2: part_e [*n_part_e, H*(K+1)]; part_a column-major [256][FN_MAX_PART] with *n_part_a rows, for fn_gat_bwd_finalize_f32. */
int fn_gat_bwd_one_f32(const float* g_out, const float* h, const float* p_sorted, const float* cdot, const float* g_s_dst,
                       const fn_edge_term* et, const float* att, int att_w, int dst_off, int src_off, const fn_gat_plan* plan,
                       float neg_slope, float* g_h, float* dz_sorted, float* g_s_orig, float* part_a, int* n_part_a,
                       float* part_e, int* n_part_e, int p_edge_major /*layout of p_sorted, as fn_gat_fwd_f32 wrote it*/,
                       float* dz_em /*nullable; non-null (four heads): the DEFERRED form, see below*/, int heads, fn_stream_t stream);
/* The deferred form (ABI 11): an OPERATOR-level form -- the engine (fn_encoder_backward) does not use it, its own deferred backward was
 * retired (FN_TUNE_RETIRED_29).  g_s_dst is not read and the forward needs no out2 / sigma.  The pass writes dz of every edge at its
 * destination-order slot, dz_em [m,4] edge-major, and leaves the two terms that need g_s_dst[t,h] = the sum of row t's contiguous
 * dz_em segment OUT of its results: g_h lacks g_s_dst[s] a_dst, and the a_dst columns of part_a are zero.  fn_gat_gsd_f32 forms
 * g_s_dst [n,4] from dz_em and overwrites those columns of part_a (rows 0 .. n_part_a-1) with the partials of dL/da_dst =
 * sum_t g_s_dst[t,h] h[t, head h's columns]; the caller adds g_s_dst[s] a_dst to g_h. */
int fn_gat_gsd_f32(const float* dz_em, const fn_gat_plan* plan, const float* h, float* g_s_dst, float* part_a, int n_part_a,
                   fn_stream_t stream);
/* c[t,h] = scale <g_out[t,h,:], out[t,h,:]>, u[t,h] = <g_out[t,h,:], out2[t,h,:]> - c[t,h] sigma[t,h] for n rows.  `out` may be the
 * level's relu(dropout(.)) output with scale = 1 - p when g_out reaches the rows through that gate only. */
int fn_gat_cu_f32(const float* g_out, const float* out, const float* out2, const float* sigma, float scale, float* c, float* u,
                  int64_t n, int heads, fn_stream_t stream);

/* Reduces the partials into g_att [H, att_w] (dst/src blocks, and the edge block in mode 2) and,
 * in mode 2, g_embW [d_e,K], g_embb [d_e].  g_att must be zero-initialised by the caller. */
int fn_gat_bwd_finalize_f32(const float* part_a, int n_part_a, const float* part_e, int n_part_e,
                            const fn_edge_term* et, const float* att, int att_w, int dst_off, int src_off,
                            float* g_att, float* g_embW, float* g_embb, int heads, fn_stream_t stream);

#define FN_MAX_PART 4096      /* upper bound on partial rows any kernel writes */

/* attention mass per SOURCE node: scatter_add(attn_probs, source) at gat2.py:165,219,268,312 */
int fn_attn_by_src_f32(const float* p_sorted, const fn_gat_plan* plan, float* attn /*[n,H]*/, int heads,
                       fn_stream_t stream);

/* s_sorted[j, pos] = <feat[eid(pos), 0:128], A[j*lda + off : +128]>, j < J <= 8, 0 at loop positions: the
 * full-width edge term of the atom and fragment graphs (edge block of `a` / `f`, gat2.py:203-208, 293-300),
 * written directly in destination-sorted order. */
int fn_row_dots_sorted_f32(const float* feat /*[m_real,128]*/, const float* A, int lda, int off, int J,
                           const fn_gat_plan* plan, float* s_sorted /*[J,m] head-major*/, fn_stream_t stream);
/* g_feat[e,:] = sum_j g_s_sorted[j, inv_d[e]] A[j]; part: column-major partial sums of g_A[j,:] */
int fn_row_dots_sorted_bwd_f32(const float* g_s_sorted, const float* feat, const float* A, int lda, int off, int J,
                               const fn_gat_plan* plan, float* g_feat, float* part, int* n_part, fn_stream_t stream);
/* x_sorted[:,pos] = x[eid(pos),:] (0 at loop positions): once per batch for the raw edge attributes */
int fn_sort_edge_attr_f32(const float* x /*[m_real,K]*/, int K, const fn_gat_plan* plan, float* x_sorted /*[K,m]*/,
                          fn_stream_t stream);
/* x_src[:,q] = x[edge at SOURCE-order position q,:] (0 for loop items): the copy the one-pass backward streams */
int fn_sort_edge_attr_src_f32(const float* x /*[m_real,K]*/, int K, const fn_gat_plan* plan, float* x_src /*[K,m]*/,
                              fn_stream_t stream);
/* out[(c / 128) * ld + off + c % 128] = sum_{r < n_rows} part[c * FN_MAX_PART + r], c < cols (partials are column-major) */
int fn_colsum_f32(const float* part, int n_rows, int cols, float* out, int ld, int off, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Node projections projection_b / projection_a / projection_fb (nn.Linear(K -> 128), gat2.py:142,189,247)
 * on the fp32 matrix cores (exact fp32 FMA chains).  K <= 168.
 *   fn_transpose_w_f32      Bt[K,128] = W[128,K]^T            (once per step per weight)
 *   fn_linear128_f32        Y[M,128] = X[M,K] Bt + bias        (forward; input gradient with Bt = W, bias = NULL)
 *   fn_linear128_wgrad_f32  dW[128,K] = dY^T X, db[128] = colsum(dY); ws holds fn_linear128_wgrad_ws(M,K) floats
 * ------------------------------------------------------------------------------------------ */
int fn_transpose_w_f32(const float* W, int K, float* Bt, fn_stream_t stream);
int fn_linear128_f32(const float* X, int K, const float* Bt, const float* bias /*nullable*/, float* Y, int64_t M,
                     const fn_act_epilogue* act_bwd /*nullable: Y *= dropout mask * (act_bwd->y > 0), the backward of
                     act(dropout(.)) fused into an input-gradient GEMM.  With relu set, act_bwd->y must be the SAVED OUTPUT
                     relu(dropout(x)) of that stream: it is positive exactly where the element was kept and passed the ReLU,
                     so the kernel scales by 1/(1-p) where y > 0 and does not replay the Philox stream*/, fn_stream_t stream);
int64_t fn_linear128_wgrad_ws(int64_t M, int K);
int fn_linear128_wgrad_f32(const float* dY, const float* X, int K, int64_t M, float* ws, float* dW, float* db,
                           fn_stream_t stream);
/* The input gradient of the layer-0 projections (csrc/input_grad.hip), what autograd returns for the INPUT of projection_b(bond nodes),
 * projection_a(x_atoms) and projection_fb(fragment-bond nodes) at gat2.py:138, 186, 241 (nn.Linear: dL/dx = dL/dy W):
 *   dx[m, k] = sum_j g[m, j] W[j, k]      g [M,128] = dL/d(projection output), 16-byte aligned; W [128,K] the Linear's weight as stored;
 *                                         1 <= K <= 168 (anything else: FN_EUNSUPPORTED); a dx row is K floats, element-aligned, unpadded
 *   dots[m]  = sum_k dx[m, k] delta[m, k] in ascending k, delta [M,K] the caller's table: gradient x input (delta = x) or integrated
 *                                         gradients' (x - x0) . grad, without dx in memory
 * dx and dots are each nullable (a task with neither, or with M = 0, launches nothing); dots needs delta.  Up to FN_MAX_DX_TASKS tasks
 * are ONE launch.  fp32 in, fp32 accumulate on the fp32 matrix cores, no atomics; every output element is a sum in a fixed order that
 * does not depend on the grid: two runs agree bit for bit.  Added under ABI 12 (nothing existing changes). */
#define FN_MAX_DX_TASKS 3
typedef struct fn_linear_dx_task {
    const float* g;            /* [M,128] */
    const float* W;            /* [128,K] */
    float* dx;                 /* [M,K], nullable */
    const float* delta;        /* [M,K], nullable when dots is */
    float* dots;               /* [M], nullable */
    int64_t M;
    int32_t K, pad_;
} fn_linear_dx_task;
int fn_linear_dx_f32(const fn_linear_dx_task* tasks, int n_tasks, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * torch_scatter.scatter_add / scatter_softmax along dim 0 on a CSR built by fn_plan_build
 * (gat2.py:234 atom->fragment sum; gat2.py:820-821 and pretrain_heads.py:93-94 pooling).
 * ------------------------------------------------------------------------------------------ */
int fn_segment_sum_f32(const float* src /*[items, src_ld >= width]*/, int64_t src_ld, const int32_t* rowptr,
                       const int32_t* perm, int32_t pos_base, float* out /*[n_seg,width]*/, int64_t n_seg,
                       int64_t width, int64_t n_items /*picks the long-segment kernel*/, fn_stream_t stream);
/* backward of the above and of index_select: out[i,:] = table[index[i],:] */
int fn_gather_rows_f32(const float* table, const int64_t* index, float* out, int64_t rows, int64_t width,
                       fn_stream_t stream);
/* probs[item,:] = softmax of logits over the items of each segment, per column (original item order) */
int fn_segment_softmax_f32(const float* logits, const int32_t* rowptr, const int32_t* perm, int32_t pos_base,
                           float* probs, int64_t n_seg, int64_t width, fn_stream_t stream);
/* g_logits = p * (g_p - sum_seg p*g_p) */
int fn_segment_softmax_bwd_f32(const float* probs, const float* g_probs, const int32_t* rowptr, const int32_t* perm,
                               int32_t pos_base, float* g_logits, int64_t n_seg, int64_t width, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Dense layers of the prediction heads, FTHead1-5 (gat2.py:569-751): Linear -> relu(dropout(.)) on [molecules, width],
 * fp32 matrix cores, 32x64 output tiles, the element-wise work fused in (csrc/dense_head.inc).  The heads' other activations, and
 * FTHead1/4's dropout(act(.)) order, run on the same kernels through the fn_*_act_f32 entry points further down (fn_head_act).
 *   fn_dense_fwd_f32   Y[M,N] = X[M,K] W[N,K]^T + bias;  with act: Y = relu?(dropout(.)), the Philox stream of
 *                      fn_dropout_act_f32 over Y's elements (act->y is ignored: the activation is applied in place)
 *   fn_dense_bwd_f32   g_y = dL/d(X W^T + bias), i.e. already through the backward of this layer's own activation;
 *                      dW[N,K] = g_y^T X;  db[N] = column sums of g_y (nullable);  g_x[M,K] = g_y W (nullable: first
 *                      layer), and with gate_scale > 0 additionally g_x = X > 0 ? g_x * gate_scale : 0 -- the backward of
 *                      the layer BELOW's relu(dropout(.)), whose saved output X is (gate_scale = 1 / (1 - p)), so the next
 *                      call receives its g_y ready.  One launch.
 * K and N multiples of 4 and <= 65536, M <= FN_DENSE_MAX_ROWS (one workgroup reduces over all of M: taller inputs go through
 * fn_gate_colsum_f32 + library GEMMs).  With M = 0, fn_dense_bwd_f32 writes zeros to dW and db.
 * ------------------------------------------------------------------------------------------ */
#define FN_DENSE_MAX_ROWS 4096
int fn_dense_fwd_f32(const float* X, const float* W, const float* bias /*nullable*/, float* Y, int64_t M, int64_t K, int64_t N,
                     const fn_act_epilogue* act /*nullable*/, fn_stream_t stream);
int fn_dense_bwd_f32(const float* g_y, const float* X, const float* W, float* g_x /*nullable, [max(M,M_out),K]*/, float gate_scale /*0: none*/,
                     float* dW, float* db /*nullable*/, int64_t M, int64_t K, int64_t N,
                     int64_t M_out /*rows [M, M_out) of g_x are set to 0 (padding rows); <= M: none*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * act(dropout(x)) between layers (gat2.py:396-397, 414-418, 436-440): Philox-4x32 mask (seven rounds, csrc/fn_internal.h) keyed by
 * (seed, offset + element/4), y = relu(keep ? x/(1-p) : 0); relu = 0 gives plain dropout.
 * Backward recomputes the mask from the same (seed, offset).
 * ------------------------------------------------------------------------------------------ */
int fn_dropout_act_f32(const float* x, float* y, int64_t numel, float p, uint64_t seed, uint64_t offset,
                       const uint64_t* offset_dev /*nullable, see fn_act_epilogue*/, int relu, fn_stream_t stream);
int fn_dropout_act_bwd_f32(const float* g_y, const float* y, float* g_x, int64_t numel, float p, uint64_t seed,
                           uint64_t offset, const uint64_t* offset_dev, int relu, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Bond-graph topology from edge_index (dataset-side; reference fragnet/dataset/data.py:116-127 get_bond_pair_bond_graph,
 * :157-182 one-bond fragments, :403-410): edge_index_bonds_graph [2, Eb] = ordered pairs (i, j) of directed bonds of a
 * molecule sharing exactly one atom, i-major / j ascending, then per molecule the mutual pairs of its two-atom
 * components (lowest atom first).  Bond id = column of the batched, molecule-contiguous edge_index [2, E];
 * atom_mol [N] = molecule of every atom (the batch vector).  Two calls because Eb is only known on the device:
 * count (fills ws, writes *total = Eb), then fill into out [2, total].  The cos(theta) attribute needs coordinates:
 * fn_bond_cos_f32 below, in the rows of this index.  ws: fn_bond_graph_ws(E, B) int32.
 * ------------------------------------------------------------------------------------------ */
/* mode FN_GRAPH_BONDS: the rule above on edge_index / batch.  mode FN_GRAPH_FBONDS: the fragment-bond graph of
 * data.py:131-154 on frag_index / frag_batch -- a molecule with exactly two connection nodes pairs the ones whose
 * (begin, end) differ, every other molecule uses the share-exactly-one rule, no extras.  (Its edge attribute is the sum
 * of the two node features, data.py:291-303, a plain gather-add.) */
#define FN_GRAPH_BONDS 0
#define FN_GRAPH_FBONDS 1
int64_t fn_bond_graph_ws(int64_t E, int64_t B);
int fn_bond_graph_count(const int64_t* edge_index /*[2,E]*/, const int64_t* atom_mol /*[N]*/, int64_t E, int64_t N, int64_t B,
                        int mode, int32_t* ws, int64_t* total /*device [1]*/, fn_stream_t stream);
int fn_bond_graph_fill(const int64_t* edge_index, const int64_t* atom_mol, int64_t E, int64_t N, int64_t B, int mode,
                       const int32_t* ws, int64_t* out /*[2,total]*/, int64_t total, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Geometry of a collated batch from atom coordinates (dataset-side; reference fragnet/dataset/data.py:185-211
 * get_edge_attr_bond_graph and :224-260 get_bond_angle_dhangle; csrc/geometry.hip).  pos [N, 3] fp32, src, dst = edge_index
 * [2, E]; u_e = (pos[src] - pos[dst]) / |.|, sigma_e = u_x + u_y + u_z, S_a = sum of sigma_e over the bonds leaving atom a in
 * ascending e.  All outputs fp32, no atomics (bit-identical from run to run), no allocation, no host synchronisation.
 *   fn_bond_cos_f32: out[j] for bond-graph edge (n1, n2) = edge_index_bonds_graph[:, j]: exactly 1 when the two bonds are the
 *     two directions of one bond (one-bond fragments), else the dot product, clamped to [-1, 1], of the unit vectors from the
 *     atom the two bonds share to their other atoms.  One flat launch.
 *   fn_pretrain_geometry_f32: bnd_lngth[e] = |pos[src] - pos[dst]|^2 (squared, as the reference stores it), bnd_angl[a] =
 *     3 S_a^2 (0 for an atom without bonds), dh_angl[e] = S_src S_dst (3 - sigma_e^2).  One workgroup per molecule: atom_mol
 *     [N] (the batch vector, values 0 .. B-1) must be non-decreasing and the bonds grouped by molecule in the same order, as
 *     every collate of this project lays a batch out.  max_atoms / max_bonds: the caller's bound on one molecule's atoms and
 *     directed bonds; above FN_GEOM_MAX_ATOMS / FN_GEOM_MAX_BONDS the call returns FN_EUNSUPPORTED (a molecule that exceeds
 *     the limits although the caller said otherwise gets NaN rows).
 * Coincident bonded atoms divide by zero as in the reference; an id outside its table gives a NaN row and is not dereferenced.
 * ------------------------------------------------------------------------------------------ */
#define FN_GEOM_MAX_ATOMS 1024
#define FN_GEOM_MAX_BONDS 4096
int fn_bond_cos_f32(const float* pos /*[N,3]*/, const int64_t* edge_index /*[2,E]*/, const int64_t* edge_index_bonds_graph /*[2,Eb]*/,
                    int64_t N, int64_t E, int64_t Eb, float* out /*[Eb]*/, fn_stream_t stream);
int fn_pretrain_geometry_f32(const float* pos /*[N,3]*/, const int64_t* edge_index /*[2,E]*/, const int64_t* atom_mol /*[N]*/, int64_t N,
                             int64_t E, int64_t B, int64_t max_atoms, int64_t max_bonds, float* bnd_lngth /*[E]*/,
                             float* bnd_angl /*[N]*/, float* dh_angl /*[E]*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Prediction-head small ops (FTHead1-5, gat2.py:631-637, 719-725, 745-751: Linear -> dropout -> act stacks on
 * [molecules, width]; the dense products themselves stay library GEMMs).
 * fn_gate_colsum_f32: backward of relu(dropout(.)) fused with the bias gradient of the Linear below it:
 *   g_x = (y > 0) ? g_y * scale : 0 (scale = 1/(1-p); the saved output encodes the mask), colsum[c] = sum_rows g_x[:, c].
 * fn_small_linear(_bwd)_f32: the last Linear of a head (n_classes <= FN_SMALL_LINEAR_MAX outputs) as one launch each
 *   way: y = x w^T + b;  g_x = g w (optionally gated by x > 0), dW = g^T x, db = colsum(g).  All sums run in a fixed order.
 * ------------------------------------------------------------------------------------------ */
#define FN_SMALL_LINEAR_MAX 16
/* Inputs taller than 2048 rows (the pretrain towers run on every edge / atom) are reduced in row chunks: pass a float
 * workspace of fn_gate_colsum_ws() / fn_small_linear_bwd_ws() elements (0 = not needed, ws may be NULL). */
int64_t fn_gate_colsum_ws(int64_t rows, int64_t cols);
int fn_gate_colsum_f32(const float* g_y /*[rows,cols]*/, const float* y /*[rows,cols]*/, float* g_x /*[rows,cols]*/,
                       float* colsum /*[cols]*/, int64_t rows, int64_t cols, float scale, float* ws, fn_stream_t stream);
int fn_small_linear_f32(const float* x /*[M,K]*/, const float* w /*[C,K]*/, const float* b /*[C] nullable*/, float* y /*[max(M,M_out),C]*/,
                        int64_t M, int64_t K, int64_t C, int64_t M_out /*rows [M, M_out) of y are set to 0: the padding
                        molecules of a static-shape batch; <= M: none*/, fn_stream_t stream);
int64_t fn_small_linear_bwd_ws(int64_t M, int64_t K, int64_t C);
int fn_small_linear_bwd_f32(const float* g /*[M,C]*/, const float* x /*[M,K]*/, const float* w /*[C,K]*/, float* g_x /*[M,K]*/,
                            float* dW /*[C,K]*/, float* db /*[C]*/, int64_t M, int64_t K, int64_t C,
                            float gate_scale /*0: none; > 0: g_x = x > 0 ? g_x * gate_scale : 0, the backward of the
                            relu(dropout(.)) that produced x (see fn_dense_bwd_f32)*/, float* ws, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The last Linear of a head + the loss on its outputs + that Linear's input gradient as ONE launch, with the sums that cross rows
 * riding in the head's first fn_dense_bwd launch (round 4).  Replaces, with the same numbers, the sequence
 *   fn_small_linear_f32 -> fn_masked_mse_f32 / fn_masked_bce_f32 -> fn_small_linear_bwd_f32
 * of a TRAINING step whose upstream gradient is d loss / d loss = 1 (train/utils.py:341 MSELoss()(out.view(-1), y), :297-304
 * compute_bce_loss, on FTHead1-5's last Linear, gat2.py:631-637).
 *   fn_small_linear_loss_f32   y[max(M,M_out),C] = x w^T + b (rows >= M: 0);  g[M,C] = d loss / d y;  g_x[M,K] = g w, gated by x > 0 when
 *                              gate_scale > 0;  loss_part[fn_small_linear_loss_ws(M_out)] = per-workgroup partial sums of the loss
 *                              (already divided by the denominator: their sum IS the loss).  kind FN_LOSS_MSE: loss =
 *                              sum_i row_w[i] sum_c (y - target)^2 / (sum_i row_w[i] * C);  FN_LOSS_BCE: BCE-with-logits averaged over
 *                              the entries with target > -0.5 and row_w > 0.  row_w [max(M,M_out)], target [max(M,M_out),C].
 *   fn_dense_bwd_tail_f32      fn_dense_bwd_f32 whose launch also runs  dW[C,K] = g^T x,  db[C] = colsum(g)  and
 *                              loss[0] = sum(loss_part)  (fixed-order sums) for the fused launch above; tail == NULL: fn_dense_bwd_f32.
 * ------------------------------------------------------------------------------------------ */
#define FN_LOSS_MSE 0
#define FN_LOSS_BCE 1
#define FN_SMALL_LINEAR_LOSS_MAX_K 1024
typedef struct fn_small_dw {
    const float* g;          /* [M,C]  d loss / d y of the last Linear */
    const float* x;          /* [M,K]  its input */
    float* dW;               /* [C,K] */
    float* db;               /* [C] */
    const float* loss_part;  /* [n_part], nullable with loss == NULL */
    float* loss;             /* [1], nullable */
    int64_t n_part, M, K, C;
} fn_small_dw;
int64_t fn_small_linear_loss_ws(int64_t M_out);
int fn_small_linear_loss_f32(const float* x /*[M,K]*/, const float* w /*[C,K]*/, const float* b /*[C] nullable*/, const float* target,
                             const float* row_w, int kind, float* y, float* g, float* g_x, float gate_scale /*0: none*/, float* loss_part,
                             int64_t M, int64_t K, int64_t C, int64_t M_out, fn_stream_t stream);
int fn_dense_bwd_tail_f32(const float* g_y, const float* X, const float* W, float* g_x, float gate_scale, float* dW, float* db,
                          int64_t M, int64_t K, int64_t N, int64_t M_out, const fn_small_dw* tail /*nullable*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The other activations of the prediction heads (finetune `act`, gat2.py:693-705) on the same kernels (csrc/head_act.inc).
 * A fn_head_act describes one hidden layer's  Linear -> dropout / act  pair, in either order:
 *   FN_ACT_DROP_THEN_ACT   y = f(u), u = dropout(z)      FTHead2/3/5 (gat2.py:631-637, 719-725)
 *   FN_ACT_ACT_THEN_DROP   y = dropout(f(u)), u = z      FTHead1/4 (gat2.py:569-587, 640-675)
 * z = X W^T + b; the mask is the Philox stream of fn_dropout_act_f32 over the layer's [M,N] elements (seed, offset, offset_dev).
 * f is torch's module: relu, silu, gelu (erf form), celu (alpha 1), selu, relu6, leakyrelu (slope 0.01), prelu (ONE slope,
 * read from prelu_w in device memory when the kernel runs).  The forward writes u to `pre` [M,N]; a backward that is handed the
 * same struct as `below` (the layer that produced its input X) reads u back, recomputes the mask from (seed, offset) and writes
 *   g_x = keep * f'(u) * (g_y W)          (torch's f' at the kinks: relu / leakyrelu / prelu / celu / selu u > 0, relu6 0 < u < 6)
 * and, for prelu, one partial sum of d loss / d slope = sum (u > 0 ? 0 : u * d loss / d f) per workgroup into `part`
 * [fn_head_act_parts()]; fn_head_act_param_grad_f32 adds all partials of a head in a fixed order (no atomics).
 *   fn_dense_fwd_act_f32            fn_dense_fwd_f32 with the activation above (act required)
 *   fn_dense_bwd_act_f32            fn_dense_bwd_tail_f32 whose input gradient goes through `below` (NULL: no gate)
 *   fn_small_linear_bwd_act_f32     fn_small_linear_bwd_f32 whose g_x goes through `below` (NULL: no gate)
 *   fn_small_linear_loss_act_f32    fn_small_linear_loss_f32 whose g_x goes through `below` (NULL: no gate)
 * fn_head_act_parts(where, rows, K): the partials one such call writes, where = FN_ACT_AT_*; rows = its M_out (M for the
 * small-linear backward, which has no padding rows).  A call with M = 0 writes none.
 * ------------------------------------------------------------------------------------------ */
#define FN_ACT_RELU 0
#define FN_ACT_SILU 1
#define FN_ACT_GELU 2
#define FN_ACT_CELU 3
#define FN_ACT_SELU 4
#define FN_ACT_RELU6 5
#define FN_ACT_LEAKYRELU 6
#define FN_ACT_PRELU 7
#define FN_ACT_DROP_THEN_ACT 0
#define FN_ACT_ACT_THEN_DROP 1
#define FN_ACT_AT_DENSE_BWD 0
#define FN_ACT_AT_SMALL_BWD 1
#define FN_ACT_AT_SMALL_LOSS 2
typedef struct fn_head_act {
    int32_t kind;               /* FN_ACT_* */
    int32_t order;              /* FN_ACT_DROP_THEN_ACT / FN_ACT_ACT_THEN_DROP */
    float p;                    /* dropout probability (0 = none) */
    int32_t pad_;
    uint64_t seed, offset;
    const uint64_t* offset_dev; /* nullable, see fn_act_epilogue */
    const float* prelu_w;       /* [1], kind FN_ACT_PRELU */
    float* pre;                 /* [M,N] the activation's argument u: written by the forward, read by the backward */
    float* part;                /* backward, kind FN_ACT_PRELU: [fn_head_act_parts()] partial sums of d loss / d slope */
} fn_head_act;
int fn_dense_fwd_act_f32(const float* X, const float* W, const float* bias /*nullable*/, float* Y, int64_t M, int64_t K, int64_t N,
                         const fn_head_act* act, fn_stream_t stream);
int fn_dense_bwd_act_f32(const float* g_y, const float* X, const float* W, float* g_x /*nullable*/, const fn_head_act* below /*nullable*/,
                         float* dW, float* db /*nullable*/, int64_t M, int64_t K, int64_t N, int64_t M_out,
                         const fn_small_dw* tail /*nullable*/, fn_stream_t stream);
int fn_small_linear_bwd_act_f32(const float* g, const float* x, const float* w, float* g_x, float* dW, float* db, int64_t M, int64_t K,
                                int64_t C, const fn_head_act* below /*nullable*/, float* ws, fn_stream_t stream);
int fn_small_linear_loss_act_f32(const float* x, const float* w, const float* b /*nullable*/, const float* target, const float* row_w,
                                 int kind, float* y, float* g, float* g_x, const fn_head_act* below /*nullable*/, float* loss_part,
                                 int64_t M, int64_t K, int64_t C, int64_t M_out, fn_stream_t stream);
int64_t fn_head_act_parts(int where, int64_t rows, int64_t K);
int fn_head_act_param_grad_f32(const float* part, int64_t n, float* grad /*[1], overwritten*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * A batch out of a resident flat store in one launch (the data side of the path: the reference's collate_fn, dataset/data.py:877-948,
 * for molecules that are kept concatenated in HBM -- fragnet_amd.dataset.FlatMolStore).  Batch molecule b = store molecule idx[b].
 *   offsets [n_spaces, B + 1] int32: first batch row of molecule b in every index space (plan.CollatedBatch.offsets: the caller has the
 *                                     store's molecule lengths on the host and builds it there)
 *   starts  [n_spaces, B]     int64: first STORE row of molecule idx[b] in every index space
 * Every field is one output tensor in index space `space`:
 *   FN_COLLATE_ROWS   dst [rows, width_words x 4 bytes] = the molecules' store rows, in batch order (features, labels: any 4-byte type)
 *   FN_COLLATE_BATCH  dst [rows] int64 = the batch molecule of every row (`batch`, `frag_batch`)
 *   FN_COLLATE_IDS    dst [width_words, rows] int64 out of src [width_words, src_rows]: index tensors (edge_index, frag_index, the two
 *                     bond-graph indices: width 2; atom_id_frag_id: width 1) whose values point into `rebase_space`: batch value =
 *                     stored value - (src_global ? first store row of the molecule there : 0) + first batch row of the molecule there
 * ------------------------------------------------------------------------------------------ */
#define FN_MAX_COLLATE_FIELDS 24
#define FN_COLLATE_ROWS 0
#define FN_COLLATE_BATCH 1
#define FN_COLLATE_IDS 2
typedef struct fn_collate_field {
    const void* src;
    void* dst;
    int64_t rows;            /* rows of dst in `space` */
    int64_t src_rows;        /* FN_COLLATE_IDS: rows of src (its second dimension) */
    int32_t width_words;     /* ROWS: 4-byte words per row; IDS: first dimension (1 or 2) */
    int32_t space, kind, rebase_space;
    int32_t src_global;
    int32_t max_seg_rows;    /* upper bound on one molecule's rows in `space` (the store's maximum); 0: unknown.  Sizes the launch only: a
                              * molecule's segment is cut into chunks that half-waves copy side by side */
} fn_collate_field;
int fn_collate_store(const fn_collate_field* fields, int n_fields, const int64_t* starts, const int32_t* offsets, int n_spaces, int64_t B,
                     const void* tables_host /*nullable: pinned host memory holding [starts | offsets]; a kernel then copies it into
                     `starts` (one device allocation that continues into `offsets`) in front of the collate launch -- no copy-engine
                     transfer on the step's stream*/, fn_stream_t stream);

/* torch.optim.Adam step (no amsgrad) on one flat fp32 tensor: finetune_gat2.py:257, pretrain_gat2.py:165.
 * `step` is the 1-based step count (bias corrections are computed on the host in double). */
int fn_adam_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                float weight_decay, int64_t step, fn_stream_t stream);
/* the same update with the 1-based step count and the learning rate read from device memory (bias corrections computed
 * in the kernel), so that the launch can sit inside a captured hipGraph and still see a new step / rate on every replay */
int fn_adam_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev /*[1]*/, float beta1,
                    float beta2, float eps, float weight_decay, const int64_t* step_dev /*[1]*/, fn_stream_t stream);

/* cat(x[src_e], x[dst_e], e_attr[e]) -> [E, 384] for the bond-length head (pretrain_heads.py:67-70) */
int fn_edge_concat_f32(const float* x /*[N,128]*/, const float* e_attr /*[E,128]*/, const int64_t* edge_index /*[2,E]*/,
                       float* out /*[E,384]*/, int64_t E, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Readout and loss.  pooled = cat(scatter_add(x_atoms, batch), scatter_add(x_frags, frag_batch)) (gat2.py:820-823)
 * as one launch into a [B,256] buffer, its backward as one launch; the molecule-weighted MSE (MSELoss of
 * train/utils.py:341 over the rows with weight 1) with its gradient in one single-block launch.
 * ------------------------------------------------------------------------------------------ */
struct fn_seg_plan;
int fn_pool_cat_f32(const float* x_atoms /*[N,128]*/, const float* x_frags /*[F,128]*/, const struct fn_seg_plan* mol_atoms,
                    const struct fn_seg_plan* mol_frags, float* out /*[B,256]*/, fn_stream_t stream);
/* leave-group-out read-out (fragment contributions: fragnet/vizualize/model_attr.py masks a fragment's atom rows AFTER the encoder):
 * out[r, 0:128] = sum of x_atoms[i, :] over the atoms i of molecule row_mol[r] with atom_group[i] != row_group[r] (row_group[r] < 0:
 * every atom; an atom_group < 0 is in no group), out[r, 128:256] = that molecule's fragment sum.  Partition and order of additions are
 * fn_pool_cat_f32's, a left-out atom enters as 0.0: a row that leaves nothing out is fn_pool_cat_f32's row of its molecule, a masked
 * row is fn_pool_cat_f32's of the table with those rows overwritten by 0.0, bit for bit.  Rows in any order, molecules may repeat;
 * R == 0 launches nothing.  row_mol must lie in [0, n_seg): the caller validates it (the kernel has no status word). */
int fn_pool_cat_groups_f32(const float* x_atoms /*[N,128]*/, const float* x_frags /*[F,128]*/, const struct fn_seg_plan* mol_atoms,
                           const struct fn_seg_plan* mol_frags, const int64_t* atom_group /*[N]*/, const int32_t* row_mol /*[R]*/,
                           const int64_t* row_group /*[R]*/, int64_t R, float* out /*[R,256]*/, fn_stream_t stream);
/* coalition read-out (fragment Shapley values: every row keeps a SET of the molecule's groups): atom_bit[i] is the position 0..63 of
 * atom i's group among its molecule's groups, < 0 for an atom in no group.  out[r, 0:128] = sum of x_atoms[i, :] over the atoms i of
 * molecule row_mol[r] with atom_bit[i] < 0 or bit atom_bit[i] of row_mask[r] set (an atom whose bit is clear enters as 0.0, its load is
 * skipped; an ungrouped atom is in every row, the empty coalition included); out[r, 128:256] = that molecule's fragment sum, never
 * masked.  Partition and order of additions are fn_pool_cat_f32's, so bit for bit: a row with every group's bit set is fn_pool_cat_f32's
 * row of its molecule, a row with all bits but one is the leave-group-out row of that group, any row is fn_pool_cat_f32's of the table
 * with the left-out atom rows overwritten by 0.0.  row_mol must be non-decreasing and lie in [0, n_seg): the caller validates it (the
 * kernel has no status word).  R == 0 launches nothing.  Form of the kernel: FN_TUNE_COALITION_STAGED. */
int fn_pool_cat_coalitions_f32(const float* x_atoms /*[N,128]*/, const float* x_frags /*[F,128]*/, const struct fn_seg_plan* mol_atoms,
                               const struct fn_seg_plan* mol_frags, const int8_t* atom_bit /*[N]*/, const int32_t* row_mol /*[R]*/,
                               const uint64_t* row_mask /*[R]*/, int64_t R, float* out /*[R,256]*/, fn_stream_t stream);
int fn_pool_cat_bwd_f32(const float* g /*[B,256]*/, const int64_t* batch /*[N]*/, const int64_t* frag_batch /*[F]*/,
                        float* g_atoms /*[N,128]*/, float* g_frags /*[F,128]*/, int64_t N, int64_t F, fn_stream_t stream);
int fn_masked_mse_f32(const float* out /*[B,T]*/, const float* y /*[B,T]*/, const float* w /*[B]*/, int64_t B, int T,
                      float* loss /*[1]*/, float* g_out /*[B,T] = dloss/dout*/, fn_stream_t stream);
/* compute_bce_loss (train/utils.py:297-304): mean over the valid entries (y > -0.5, w > 0) of BCE-with-logits(out, max(y, 0)),
 * and its gradient; one single-block launch (B*T is ~12 k for Tox21 at batch 1024). */
int fn_masked_bce_f32(const float* out /*[B,T]*/, const float* y /*[B,T]*/, const float* w /*[B]*/, int64_t B, int T,
                      float* loss /*[1]*/, float* g_out /*[B,T]*/, fn_stream_t stream);
/* loss = sum_k coef_k * masked_mse_k with coef_k = tasks[k].coef * (scale_dev[tasks[k].scale_idx] if scale_idx >= 0 else 1):
 * the pretrain loss 2*MSE(dihedral) + MSE(angle) + MSE(energy) (pretrain_utils.py:9-31) with the per-rank weights of the
 * per-edge / per-atom means, and all three gradients, in two multi-block launches.  ws: fn_masked_mse_multi_ws(n) floats. */
typedef struct fn_mse_task {
    const float *out, *y, *w;   /* [B,T], [B,T], [B] */
    float* g_out;               /* [B,T] = d loss / d out */
    int64_t B;
    int32_t T, scale_idx;
    float coef, pad_;
} fn_mse_task;
int64_t fn_masked_mse_multi_ws(int n_tasks);
int fn_masked_mse_multi_f32(const fn_mse_task* tasks, int n_tasks /*<= 4*/, const float* scale_dev /*nullable*/, float* ws,
                            float* loss /*[1]*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Static-shape staging for hipGraph replay.  A training step captured in a hipGraph has fixed tensor shapes, so
 * every batch (the dict of dataset/data.py:931-948) is copied into fixed-capacity buffers and the tail of each
 * buffer is filled with PADDING that is itself a valid, disconnected piece of graph: zero feature rows, and index
 * values pointing at the last `pad_mod` slots of the target index space (pad value at position i =
 * pad_hi - (i - n_real) % pad_mod: the first padding item points at the last slot), so padding only ever talks to padding and
 * in-degrees stay small.  One launch, all fields.
 * ------------------------------------------------------------------------------------------ */
#define FN_MAX_STAGE_FIELDS 40
#define FN_STAGE_ROWS 0 /* float32 [cap,width]  <- [n_real,width], zero rows after                         */
#define FN_STAGE_IDS 1  /* int64   [cap]        <- [n_real], pad ids after                                 */
#define FN_STAGE_COLS 2 /* int64   [2,cap]      <- [2,n_real] (edge_index layout), pad ids in both rows    */
#define FN_STAGE_MASK 3 /* float32 [cap]        =  1 for i < n_real, 0 after (loss weights); src unused    */
#define FN_STAGE_COUNT 4 /* int32 [1]           =  n_real (device-side copy of a count for the fused encoder)  */
#define FN_STAGE_ZERO 6  /* int32 [cap]         =  0 (workspace of a captured fn_plan_build, see FN_PLAN_PREZEROED); src unused */
#define FN_STAGE_OFFSETS 7 /* int32 [width][cap+1] <- [width][n_real+1]: per-molecule offsets of `width` index spaces (fn_mol_layout);
                            *                       entries behind molecule n_real repeat the space's total */
#define FN_STAGE_BUMP 5  /* int64 [1]          +=  n_real: a device-side counter of a captured step (Philox blocks, optimiser steps)
                          *                       advanced by the staging launch that precedes every replay instead of by a launch of its own */
#define FN_STAGE_ROWS_I64 8 /* int64 [cap,width]   <- [n_real,width], zero rows after (the second input of a pair model: gene_expr, protein
                             *                       tokens); FN_STAGE_ROWS's checks, and src and dst 8-byte aligned */
typedef struct fn_stage_field {
    const void* src;
    void* dst;
    int64_t n_real, cap;
    int32_t width, kind;
    int64_t pad_hi, pad_mod;
} fn_stage_field;
int fn_stage_padded(const fn_stage_field* fields, int n_fields, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PretrainTask's tall towers (pretrain_heads.py:33-58, 77-88: `PretrainTask(128, 1)`, L = 2): Linear(128 -> 64) -> ReLU ->
 * Linear(64 -> 32) -> ReLU -> Linear(32 -> 1) on every atom (bond angle) / every directed bond (dihedral).  One launch each way
 * for up to FN_MAX_TOWERS towers (+ one reduction launch in the backward): the 41 KB of weights live in LDS, a workgroup walks
 * 32-row tiles, the hidden rows never leave the CU in the forward except as the saved h1 / h2.
 * fn_tower_bwd_f32: g_x [M,128] = dL/dx (nullable), g_w* / g_b* = parameter gradients (overwritten), ws = fn_tower_bwd_ws() floats.
 * ------------------------------------------------------------------------------------------ */
#define FN_MAX_TOWERS 4
typedef struct fn_tower {
    const float* x;                              /* [M,128] */
    const float *w1, *b1, *w2, *b2, *w3, *b3;    /* [64,128], [64], [32,64], [32], [1,32], [1] */
    float *h1, *h2;                              /* [M,64], [M,32]: relu outputs, written by the forward, read by the backward */
    float* out;                                  /* [M,1] (forward) */
    int64_t M;
    const float* g_out;                          /* [M,1] (backward) */
    float* g_x;
    float *g_w1, *g_b1, *g_w2, *g_b2, *g_w3, *g_b3;
} fn_tower;
int fn_tower_fwd_f32(const fn_tower* towers, int n, fn_stream_t stream);
int64_t fn_tower_bwd_ws(const fn_tower* towers, int n);
int fn_tower_bwd_f32(const fn_tower* towers, int n, float* ws, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Encoder engine: the reference's FragNet.forward (gat2.py:381-442: L x FragNetLayerA + act(dropout(.))) and
 * its backward pass as one call each.  The host side only walks the layers and enqueues kernels on `stream`;
 * nothing is allocated, nothing synchronises.  `ws` keeps the activations the backward pass reads.
 * Gradient pointers in `grads[l]` that the pass does not produce are left untouched: `f` for every layer but the
 * last (the fragment-graph output of inner layers is dead in the reference).
 * ------------------------------------------------------------------------------------------ */
#define FN_MAX_LAYERS 8

typedef struct fn_layer_weights {          /* parameters of one FragNetLayerA, or their gradients */
    float *proj_b_w, *proj_b_b;            /* projection_b  [128,Kb], [128]  (gat2.py:88)  */
    float *proj_a_w, *proj_a_b;            /* projection_a  [128,Ka], [128]  (gat2.py:95)  */
    float *proj_fb_w, *proj_fb_b;          /* projection_fb [128,Kfb], [128] (gat2.py:89)  */
    float *emb_b_w, *emb_b_b;              /* edge_attr_bond_embed  [d,1], [d]  (gat2.py:91) */
    float *emb_fb_w, *emb_fb_b;            /* edge_attr_fbond_embed [d,Kf], [d] (gat2.py:92) */
    float *a_b, *a, *f, *f_a_b;            /* attention vectors (gat2.py:98-109) */
} fn_layer_weights;

/* a slice of FlatAdam's buffers with the step count and the learning rate in device memory (see fn_adam_dev_f32) */
typedef struct fn_adam_slice {
    float* p;  const float* g;  float* m;  float* v;
    int64_t n;                       /* elements; p, g, m, v 16-byte aligned */
    const float* lr_dev;  const int64_t* step_dev;
    float beta1, beta2, eps, weight_decay;
    int32_t launched, pad_;          /* OUT (fn_encoder.adam_rider only): set to 1 by fn_encoder_backward once the launch that carries
                                      * the slice has been enqueued; the caller clears it before the call and updates the slice itself
                                      * when it is still 0 afterwards (ABI 11) */
} fn_adam_slice;

typedef struct fn_encoder {
    int32_t n_layers, heads;
    int32_t k_atom0, k_bond0, k_fbond0;    /* layer-0 feature widths (167, 17, 6); 128 afterwards */
    int32_t k_fattr;                       /* width of edge_attr_fbonds (6) */
    int32_t training;
    int32_t variant;                       /* 0: gat2; 1: gat2_lite (gat2_lite.py: every layer stops after the atom -> fragment sum;
                                            * out_fbond is not written, out_frags = relu(dropout(fragment sums)));
                                            * 2: gat2_edge (gat2_edge.py: no fragment-bond graph; the fragment graph's edge term is
                                            * <Linear(k_fattr -> 128)(cnx_attr), f[:, d:d+128]> with the Linear in w[l].emb_fb_w/_b
                                            * ([128, k_fattr], [128]) and cnx_attr sorted by the FRAGMENT graph in fattr_sorted
                                            * [k_fattr, frag.m]; proj_fb_* and f_a_b are placeholders, out_fbond is not written) */
    float drop_p, pad2_;
    uint64_t seed, offset;                 /* Philox stream; fn_encoder_rng_blocks() offsets are consumed */
    const uint64_t* offset_dev;            /* nullable device counter added to offset at run time (hipGraph replays) */
    int64_t N, E, F, EF;
    fn_gat_plan bond, atom, fbond, frag;
    fn_seg_plan a2f;
    const float *x_atoms, *bond_nodes, *fbond_nodes;     /* layer-0 inputs */
    const float *cos_sorted, *fattr_sorted;              /* fn_sort_edge_attr_f32 outputs: [1, bond.m] and [k_fattr, fbond.m] */
    const float *cos_raw, *fattr_raw;                    /* nullable.  When set (edge order of the batch: [bond.m_real] and
                                                          * [fbond.m_real, k_fattr]) fn_encoder_forward permutes them into
                                                          * cos_sorted / fattr_sorted itself, inside its one prologue launch;
                                                          * the two *_sorted buffers must then be writable */
    fn_layer_weights w[FN_MAX_LAYERS];
    float* ws;
    int64_t ws_floats;                     /* >= fn_encoder_ws_floats() */
    /* Molecule CSRs (optional; n_mols = 0: absent).  collate_fn concatenates molecules, so the atoms / bonds / fragments /
     * connections / graph edges of molecule i are contiguous ranges (dataset/data.py:877-948).  They drive the molecule-resident
     * fragment tail (below) and the padding-row skip (FN_TUNE_PAD_SKIP). */
    fn_seg_plan mol_atoms, mol_frags;      /* atoms / fragments keyed by molecule (batch, frag_batch: gat2.py:820-821) */
    int64_t n_mols;
    const int32_t* counts_dev;             /* nullable device [1]: number of REAL molecules (the first ones) when the batch is
                                            * padded to static shapes (fn_stage_padded, FN_STAGE_COUNT); outputs of padding rows
                                            * are zero */
    int32_t* status;                       /* nullable device word, bits OR-ed in on malformed batches */
    /* Fused fragment tail (csrc/mol_tail.inc).  mol_contiguous: the caller's word that the batch has collate_fn's layout
     * (molecules concatenated: every index range of a molecule is contiguous and the molecule CSRs above are given).  Then the
     * last layer's atom -> fragment sum, fragment-graph attention and -- when `pooled` is set -- the readout
     * cat(scatter_add(out_atoms, batch), scatter_add(out_frags, frag_batch)) [n_mols, 256] (gat2.py:820-823) run as ONE
     * molecule-resident launch, and their backward (with dL/d(pooled) in `g_pooled`, nullable, added to g_atoms / g_frags) as
     * one more.  fn_encoder_fused_tail() says whether a descriptor takes that path; `pooled` / `g_pooled` must be NULL if not. */
    int32_t mol_contiguous;
    /* no_backward (was padding: 0 keeps the old behaviour): the caller's word that no fn_encoder_backward will follow this
     * fn_encoder_forward (torch.no_grad() / nothing requires a gradient).  An EVALUATION pass (training == 0) then saves nothing
     * for one: the attention probabilities of its levels are not stored, nor the raw bond rows once their only forward reader --
     * the atom graph's edge term -- was folded into the bond level's launch (FN_TUNE_FUSE_ROWDOTS).  Outputs are bit-identical;
     * fn_encoder_backward on such a descriptor returns FN_EINVAL.  Ignored by training passes. */
    int32_t no_backward;
    float* pooled;
    const float* g_pooled;
    /* fn_encoder_backward only, nullable: an Adam update (fn_adam_dev_f32's arithmetic) of a slice of the flat parameter buffer whose
     * gradients were complete before this backward pass began -- the prediction head's -- rides in the pass's last launch (the
     * deferred reductions), independent of everything that launch reduces.  The caller's own Adam launch then covers the rest
     * (torch.optim.Adam is element-wise: finetune_gat2.py:257).  ABI 10. */
    struct fn_adam_slice* adam_rider;
} fn_encoder;

int fn_encoder_fused_tail(const fn_encoder* e);      /* 1: fn_encoder_forward / _backward run the fused fragment tail */

int64_t fn_encoder_ws_floats(const fn_encoder* e);
int64_t fn_encoder_bwd_ws_floats(const fn_encoder* e);
uint64_t fn_encoder_rng_blocks(const fn_encoder* e);
/* out_bond and out_fbond may both be NULL: the caller reads neither (a finetune head pools atoms and fragments only, gat2.py:816-826)
 * and the last layer's activated bond / fragment-bond rows are not stored (the levels themselves still run: the atom and fragment
 * graphs read their raw rows).  The other outputs do not change a bit. */
int fn_encoder_forward(const fn_encoder* e, float* out_atoms /*[N,128]*/, float* out_frags /*[F,128]*/,
                       float* out_bond /*[E,128], nullable*/, float* out_fbond /*[EF,128], nullable*/, fn_stream_t stream);
/* Row masks of an evaluation pass (leave-one-out attribution; the reference's bond_mask / atom_mask_individual / frag_bond_mask,
 * gat2.py:173-176, 227-231, 275-278, as a per-batch input instead of one scalar index per layer).  One byte per row, non-zero = the
 * row is ZERO for every reader, in EVERY layer: the bond level's new_bond [E], the atom level's x_atoms_new [N], the fragment-bond
 * level's new_fbond [EF] -- set on the finished row inside the level's kernel, before the raw store, the atom graph's edge term and the
 * activated store.  Each array is nullable (no masked row in that index space).  A bond is the two directed rows 2k, 2k + 1 of its
 * molecule, and so is a fragment connection: whoever fills the arrays sets both (fn_loo_row_masks_u8 does).  There is no fragment mask.
 * m == NULL or three NULL arrays: fn_encoder_forward itself, bit for bit.  Otherwise the pass needs variant == 0 (FN_EUNSUPPORTED),
 * training == 0 and no_backward == 1 (FN_EINVAL) and heads == 4 (FN_EUNSUPPORTED): refused before anything is launched.  ABI 12. */
typedef struct fn_row_masks {
    const uint8_t *atoms /*[N]*/, *bonds /*[E]*/, *fbonds /*[EF]*/;
} fn_row_masks;
int fn_encoder_forward_masked(const fn_encoder* e, const fn_row_masks* m, float* out_atoms, float* out_frags, float* out_bond,
                              float* out_fbond, fn_stream_t stream);
/* Attention read-out of an evaluation pass: the LAST layer's summed_attn_weights_atoms / _frags / _bonds / _fbonds of the reference,
 * scatter_add(attn_probs, source) at gat2.py:219, 312, 165, 268 -- what fragnet/vizualize/model.py returns and viz.py draws.  Each
 * pointer is nullable (that level's sums are not wanted); a tensor has one row per node of its level, [n, heads] floats, and rows
 * without out-edges are 0 (the reference's scatter_add without dim_size stops at source.max() + 1: its tensor is a prefix of this one).
 * The pass is fn_encoder_forward's, launch for launch, except that the last layer's bond, fragment-bond, atom and fragment levels store
 * their probabilities under no_backward too (same kernels: one more store per edge; the outputs are the plain pass's bits), plus ONE
 * launch behind the last level (csrc/attn_readout.hip): attn[s][h] = sum_k |p[h m + dpos_s[beg_s + k]]| in ascending by-source position
 * = ascending original edge id (the atom level's self loops last), the reference's sequential order -- reproducible bit for bit and
 * equal to fn_attn_by_src_f32 on the same probabilities.  A level without edges reads nothing and zero-fills its tensor in that launch.
 * r == NULL or four NULL pointers: fn_encoder_forward itself, bit for bit.  Otherwise the pass needs variant == 0 (FN_EUNSUPPORTED:
 * the reference's gat2_lite / gat2_edge Viz classes cannot run) and training == 0 (FN_EINVAL): refused before anything is launched.
 * Both values of no_backward and every head count fn_encoder_forward evaluates are accepted.  There is no read-out of a masked pass
 * (fn_encoder_forward_masked takes none).  Inner layers store and sum nothing: the reference returns the last layer's only.  ABI 12. */
typedef struct fn_attn_readout {
    float *atoms /*[N,H]*/, *frags /*[F,H]*/, *bonds /*[E,H]*/, *fbonds /*[EF,H]*/;
} fn_attn_readout;
int fn_encoder_forward_attn(const fn_encoder* e, const fn_attn_readout* r, float* out_atoms, float* out_frags, float* out_bond,
                            float* out_fbond, fn_stream_t stream);
/* Input gate of the atom features (masked-atom pretraining, the reference's FragNetPreTrainMasked2, pretrain_heads.py:187-236): one
 * byte per row of x_atoms, ZERO = the row reads as zero for every consumer, non-zero = kept.  The gate is applied BEFORE the input
 * dropout (the reference zeroes the rows, then FragNet.forward drops out), inside the prologue's existing pass over x_atoms: that
 * block range writes dropout(gate(x_atoms)) -- with p_eff == 0 (evaluation, or drop_p == 0) a gated copy -- and layer 0's projection
 * and its weight-gradient product read that copy; no launch is added, and kept rows draw the dropout bits they draw without a gate.
 * Training passes (fn_encoder_backward may follow: the pass remembers per workspace that it was gated) and evaluation passes with both
 * values of no_backward.  With p_eff == 0 the gated copy lives behind the plain workspace: e->ws_floats must be at least
 * fn_encoder_keep_ws_floats(e) (fn_encoder_ws_floats(e) + N * k_atom0, rounded as the workspace rounds).
 * keep == NULL: fn_encoder_forward itself, bit for bit.  Otherwise variant == 0 is needed (FN_EUNSUPPORTED, before anything is
 * launched), and fn_encoder_backward_inputs after a gated forward returns FN_EUNSUPPORTED (no input gradients of masked passes).
 * ABI 12. */
int64_t fn_encoder_keep_ws_floats(const fn_encoder* e);
int fn_encoder_forward_keep(const fn_encoder* e, const uint8_t* keep_atoms /*[N], nullable*/, float* out_atoms, float* out_frags,
                            float* out_bond, float* out_fbond, fn_stream_t stream);
/* An exact-count sample of rows without replacement, drawn on the device in ONE launch (csrc/row_sample.hip).  Of the n real rows
 * of a table of cap rows, k = (int)((double)n * keep_frac) are kept -- Python's int(n * keep_frac), the same IEEE double product:
 * out[i] = 1 for i < n iff fewer than k rows j < n have (key_j, j) < (key_i, i) lexicographically (the k smallest keys, ties broken
 * by row index: exactly k ones, a function of the keys alone), else 0; padding rows n <= i < cap get 1.  n_dev (nullable device int32)
 * replaces n when given -- the real row count of a padded batch -- and is clamped to [0, cap] before use.  cap <= 2^24; keep_frac in
 * [0, 1]; anything else is FN_EINVAL.
 * fn_select_rows_u8 takes the keys [cap] (those of rows >= n are not read).  fn_sample_rows_u8 generates them: the key of row i is
 * word i % 4 of Philox block offset + *offset_dev + i / 4 under `seed` -- fn_dropout_act_f32's convention -- so one draw consumes
 * (cap + 3) / 4 blocks of whatever stream (seed, counter) the caller dedicates to it.  ABI 12. */
int fn_select_rows_u8(const uint32_t* keys /*[cap]*/, int64_t cap, int64_t n, const int32_t* n_dev, double keep_frac, uint8_t* out /*[cap]*/,
                      fn_stream_t stream);
int fn_sample_rows_u8(uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int64_t cap, int64_t n, const int32_t* n_dev,
                      double keep_frac, uint8_t* out /*[cap]*/, fn_stream_t stream);
/* The three masks of a batch of leave-one-out replicas, zero-filled and set in ONE launch. replicas: int32 [n_mols][2] = (kind, local
 * index) of molecule i of the batch; kind 0 masks nothing, 1 the atom `index`, 2 the bond `index` (directed rows 2 index, 2 index + 1),
 * 3 the fragment connection `index` (rows 2 index, 2 index + 1), all local to the molecule.  *_off: int32 [n_mols + 1], first row of
 * molecule i in the atom / directed-bond / directed-fragment-connection space (rows of a CollatedBatch's offsets table); they must end
 * at N / E / EF.  The masks are 16-byte aligned device arrays of N / E / EF bytes.  A replica whose kind is not 0..3 or whose rows are
 * not all inside its molecule writes nothing and ORs FN_STATUS_BAD_REPLICA into *status (device word, required). */
#define FN_STATUS_BAD_REPLICA 8
int fn_loo_row_masks_u8(const int32_t* replicas, int64_t n_mols, const int32_t* atom_off, const int32_t* bond_off,
                        const int32_t* fbond_off, uint8_t* mask_atoms, int64_t N, uint8_t* mask_bonds, int64_t E,
                        uint8_t* mask_fbonds, int64_t EF, int32_t* status, fn_stream_t stream);
/* g_* are dL/d(out_*) (nullable = zero); out_* are the forward outputs (needed for the ReLU mask; out_bond / out_fbond may be
 * NULL where the forward pass was given NULL -- their gradients must then be NULL too). */
int fn_encoder_backward(const fn_encoder* e, const float* out_atoms, const float* out_frags, const float* out_bond,
                        const float* out_fbond, const float* g_atoms, const float* g_frags, const float* g_bond,
                        const float* g_fbond, const fn_layer_weights* grads /*[n_layers]*/, float* scratch,
                        int64_t scratch_floats, fn_stream_t stream);
/* Gradients with respect to the encoder's three INPUT feature tables, after fn_encoder_backward: x_atoms feeds projection_a only
 * (gat2.py:186), the bond nodes projection_b (gat2.py:138), the fragment-bond nodes projection_fb (gat2.py:241) -- all of layer 0, whose
 * dL/d(projection output) rows fn_encoder_backward leaves in its scratch (per layer and level, never reused).  This call multiplies them
 * by the three weights in ONE launch (fn_linear_dx_f32's kernel).  e / scratch / scratch_floats: those of the fn_encoder_backward call
 * that precedes it on the same stream, untouched in between.  in: up to three dx tables and up to three (delta, dots) pairs as in
 * fn_linear_dx_task, every pointer nullable (all NULL: nothing is launched).
 * A separate call and not an argument of fn_encoder_backward: that call's signature, launches and bits stay what they were for every
 * caller that differentiates the parameters only.
 * Rows of a level the backward pass did not reach (no gradient arrived there) are not written by it: a caller that cannot rule that out
 * hands fn_encoder_backward a zero-filled scratch, and reads zeros here.
 * Refused before anything is launched: variant 2, gat2_edge (FN_EUNSUPPORTED); fragment-bond outputs with variant 1, gat2_lite, which has
 * no fragment-bond level (FN_EINVAL); a training pass with drop_p > 0 (FN_EUNSUPPORTED: the input dropout's gate on x_atoms, gat2.py:396,
 * would have to be replayed); a descriptor whose evaluation forward ran with no_backward (FN_EINVAL); FN_TUNE_BWD_ONE
 * changed since the forward (FN_EINVAL).  Added under ABI 12. */
typedef struct fn_input_grads {
    float *dx_atoms /*[N,k_atom0]*/, *dx_bonds /*[E,k_bond0]*/, *dx_fbonds /*[EF,k_fbond0]*/;
    const float *delta_atoms, *delta_bonds, *delta_fbonds;     /* same shapes */
    float *dots_atoms /*[N]*/, *dots_bonds /*[E]*/, *dots_fbonds /*[EF]*/;
} fn_input_grads;
int fn_encoder_backward_inputs(const fn_encoder* e, const float* scratch, int64_t scratch_floats, const fn_input_grads* in,
                               fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Cancer drug response model, CDRP (reference model/cdrp/model.py: CDRPModel = FragNet encoder + MLP(gene_dim) cell-line tower + the
 * pair head fc2(fc1(cat(drug_enc, cell_enc)))); csrc/cdrp.hip, the pair head csrc/pair_head.hip.  Entry points added under ABI 12
 * (nothing existing changes).
 * fp32 accumulate on the fp32 matrix cores, no atomics, sums over rows in a fixed order.  M <= FN_DENSE_MAX_ROWS throughout; M = 0 is
 * legal: the forward calls launch nothing, the backward calls write zeros to the weight-gradient outputs.
 *   fn_cdrp_gene_fwd_f32   Y[M,N] = relu(float(G[M,K]) W[N,K]^T + bias): the tower's first Linear on the int64 rows collate_fn_cdrp
 *                          produces (the conversion, round to nearest like .float(), is part of the load).  K >= 1 is ANY length (903 in
 *                          the reference's configs) -- rows of G and W need element alignment only, the K tail is handled in the kernel,
 *                          nothing is padded; N a multiple of 4; K, N <= 65536.
 *   fn_cdrp_gene_bwd_f32   dW[N,K] = g^T float(G),  db[N] = column sums of g (nullable).  g = g_y when y_gate == NULL: g_y is then already
 *                          through this layer's ReLU (what fn_dense_bwd_f32 of the layer above hands down with gate_scale = 1);
 *                          with y_gate = the saved output Y, g = g_y where Y > 0 and 0 elsewhere.  No input gradient: gene_expr is data.
 * Tower layers 2-4 (1024 -> 256 -> 64 -> 256, ReLU after each, no dropout) are fn_dense_fwd_f32 (ReLU epilogue, p = 0) and
 * fn_dense_bwd_f32 (gate_scale = 1).
 * Attributions of gene_expr (gradient x input and integrated gradients over a straight path; entry points added under ABI 12, nothing
 * existing changes).  M = C S rows: row r is path node j = r % S of cell line c = r / S.  S >= 1, M <= FN_DENSE_MAX_ROWS, C = 0 is legal
 * (nothing is launched or written); K, N and the alignment rules as for fn_cdrp_gene_fwd_f32.
 *   fn_cdrp_gene_fwd_path_f32  Y[M,N] = relu(X W[N,K]^T + bias) with X[r,k] = base[k] + alpha[j] (float(G[c,k]) - base[k]) formed in the load
 *                          from the int64 rows G[C,K], base[K] (nullable: zeros) and alpha[S]; no float [M,K] table is written.  With
 *                          S = 1, alpha = {1} and base == NULL the result is fn_cdrp_gene_fwd_f32's, bit for bit.
 *   fn_cdrp_gene_dx_f32    the layer's input gradient dX[r,k] = sum_n g[r,n] W[n,k] (g gated as in fn_cdrp_gene_bwd_f32: y_gate == NULL
 *                          means g_y is already through the ReLU), folded where it is produced:
 *                          attr[c,k] = (float(G[c,k]) - base[k]) * grad_mean[c,k],  grad_mean[c,k] = (sum_j dX[c S + j, k]) / S,
 *                          the S rows of a cell line added in ascending j.  grad_mean [C,K] is stored only when non-null; the [M,K]
 *                          gradient table never is.  With S = 1 this is gradient x input.  One launch.
 *   fn_cdrp_pair_fwd_f32  h[M,H] = drug[M,Kd] W1[:, :Kd]^T + cell[M,Kc] W1[:, Kd:]^T + b1 (W1 [H, Kd + Kc]; no cat is written; h is saved
 *                          for the backward), out[M] = h w2 + b2 (w2 [C,H], C = 1).  With target [M] (nullable): g[M] = d MSE / d out =
 *                          2 (out - target) / M and loss_part[fn_cdrp_pair_loss_ws(M)] = per-workgroup partial sums of mean((out - target)^2),
 *                          whose sum in order is the loss.  One launch.
 *   fn_cdrp_pair_bwd_f32   from g[M] = d loss / d out (the forward's, or the caller's): dW2[C,H], db2[C], dW1[H, Kd + Kc], db1[H],
 *                          g_drug[M,Kd], and g_cell[M,Kc] ALREADY through the backward of the ReLU that produced cell (0 where cell <= 0),
 *                          so the tower's fn_dense_bwd_f32 receives its g_y ready.  loss != NULL: loss[0] = sum of the n_part partials in a
 *                          fixed order.  One launch.
 * The pair head is built for the reference's widths only, Kd = Kc = 256, H = 128, C = 1: anything else returns FN_EUNSUPPORTED (with the
 * reason in fn_last_error) before anything is launched or written.  drug, cell, h, W1, g_drug, g_cell, dW1: 16-byte aligned.
 * fn_cdrp_pair_* and fn_dta_pair_* (below) are the two instances of ONE kernel template (csrc/pair_head.hip), <second width, gate> =
 * <256, true> and <300, false>: the same arguments, checks, tile shapes and order of operations; they differ in the second input's width
 * and in whether its gradient is gated, in nothing else.
 * ------------------------------------------------------------------------------------------ */
int fn_cdrp_gene_fwd_f32(const int64_t* G, const float* W, const float* bias /*nullable*/, float* Y, int64_t M, int64_t K, int64_t N,
                         fn_stream_t stream);
int fn_cdrp_gene_bwd_f32(const float* g_y, const float* y_gate /*nullable*/, const int64_t* G, float* dW, float* db /*nullable*/, int64_t M,
                         int64_t K, int64_t N, fn_stream_t stream);
int fn_cdrp_gene_fwd_path_f32(const int64_t* G, const float* base /*nullable*/, const float* alpha, const float* W, const float* bias /*nullable*/,
                              float* Y, int64_t C, int64_t S, int64_t K, int64_t N, fn_stream_t stream);
int fn_cdrp_gene_dx_f32(const float* g_y, const float* y_gate /*nullable*/, const float* W, const int64_t* G, const float* base /*nullable*/,
                        float* attr, float* grad_mean /*nullable*/, int64_t C, int64_t S, int64_t K, int64_t N, fn_stream_t stream);
int64_t fn_cdrp_pair_loss_ws(int64_t M);
int fn_cdrp_pair_fwd_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                         const float* target /*nullable*/, float* h, float* out, float* g /*nullable without target*/,
                         float* loss_part /*nullable without target*/, int64_t M, int64_t Kd, int64_t Kc, int64_t H, int64_t C,
                         fn_stream_t stream);
int fn_cdrp_pair_bwd_f32(const float* g, const float* drug, const float* cell, const float* h, const float* W1, const float* w2,
                         float* g_drug, float* g_cell, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part /*nullable*/,
                         int64_t n_part, float* loss /*nullable*/, int64_t M, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream);
/* fn_cdrp_pair_fwd_rows_f32 / fn_dta_pair_fwd_rows_f32 (added under ABI 12, nothing existing changes): fn_*_pair_fwd_f32 with a
 * DEVICE-side count of the real rows, for the M = capacity rows of a static-shape step: real_rows = the int32 word the staging launch
 * writes (FN_STAGE_COUNT), n = *real_rows clamped to [0, M].  Rows i < n: out, h, g[i] = 2 (out - target) / n, partials divided by n;
 * rows i >= n: out and h written, g[i] = 0 exactly, no share of the loss; n = 0: loss 0, every g 0, no division.  fn_*_pair_bwd_f32 is
 * called as before, on all M rows: a zero g makes every term of a padding row an exact zero (finite inputs), its g_drug / g_cell rows
 * included.  real_rows == NULL: fn_*_pair_fwd_f32, bit for bit.  real_rows without a target: FN_EINVAL. */
int fn_cdrp_pair_fwd_rows_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                              const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kc,
                              int64_t H, int64_t C, const int32_t* real_rows /*nullable, device*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Drug-target affinity model, DTA (reference model/dta/model.py: DTAModel2 = FragNet encoder + protein tower Embedding(V, D) ->
 * Conv1d(L -> F, KS) along the embedding axis -> Linear(F J, 300), J = D - KS + 1, no activation anywhere -> the pair head
 * fc2(fc1(cat(drug_enc, xt)))); csrc/dta.hip, the pair head csrc/pair_head.hip.  Entry points added under ABI 12 (nothing existing
 * changes).  fp32 accumulate, no atomics, every sum over positions, samples or rows in a fixed order.  M <= FN_DENSE_MAX_ROWS
 * throughout; M = 0 is legal: the forward calls launch nothing, the backward calls write zeros to the gradient outputs.
 * The convolution runs in its histogram form (the layer is linear in the V-row table E):
 *     A[b, v, f, k] = sum of W[f, c, k] over the positions c with tok[b, c] = v;   conv[b, f, j] = bias[f] + sum_v sum_k A[b, v, f, k] E[v, j + k]
 *   fn_dta_conv_fwd_f32    tok[M,L] int64 (what collate_fn_dta produces), E[V,D], W[F,L,KS], bias[F] -> conv[M, F J], laid out as the
 *                          reference's conv_xt.view(-1, F J) so that the dense layer reads it in place, and A[M, V, F KS] (note the
 *                          order: v outermost), saved for the backward.  Two launches (histogram, contraction).
 *   fn_dta_conv_bwd_f32    from g_conv[M, F J]: dW[F,L,KS], dbias[F], dE[V,D]; no input gradient (tokens are data).  Three launches:
 *                          per sample G[b, v, f, k] = sum_j g[b, f, j] E[v, j + k] and the sample's shares of dE and dbias; the gather
 *                          dW[f, c, k] = sum_b G[b, tok[b, c], f, k] (samples in order; more than 32 samples: up to 16 partial sums); the
 *                          sums of the partials in order.  ws: fn_dta_conv_bwd_ws(M, L, D, V) floats, 16-byte aligned.
 * Built instance: F = 32, KS = 8, 1 <= V <= 32 -- anything else returns FN_EUNSUPPORTED before anything is launched or written.
 * Run-time: 1 <= L <= 4096 and ANY 8 <= D <= 512 (no multiple-of-4 rule: E, W, conv, g_conv, dE need element alignment only, the tails
 * are masked, nothing is padded in memory); outside: FN_EINVAL.  A, dW, ws: 16-byte aligned.
 * A token outside [0, V) is never used to index memory: it falls into no bin (its position contributes nothing to conv) and its
 * dW[:, c, :] terms are absent (0 from every sample that has such a token there).  torch raises instead; collate_fn_dta checks on the host.
 *   fn_dta_pair_fwd_f32 / fn_dta_pair_bwd_f32 / fn_dta_pair_loss_ws
 *                          the <300, false> instance of the pair head (fn_cdrp_pair_*_f32 above is <256, true>), same arguments and
 *                          contract, for Kd = 256, Kx = 300, H = 128, C = 1 (W1 [128, 556]; 300 = 18 x 16 + 12: the reduction's tail is
 *                          masked) with ONE difference: g_xt[M,300] is NOT gated -- xt is the output of a Linear, not of a ReLU.  Other widths: FN_EUNSUPPORTED.  drug, xt, h, W1, g_drug, g_xt,
 *                          dW1: 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int fn_dta_conv_fwd_f32(const int64_t* tok, const float* E, const float* W, const float* bias, float* A, float* conv, int64_t M, int64_t L,
                        int64_t D, int64_t V, int64_t F, int64_t KS, fn_stream_t stream);
int64_t fn_dta_conv_bwd_ws(int64_t M, int64_t L, int64_t D, int64_t V);
int fn_dta_conv_bwd_f32(const float* g_conv, const int64_t* tok, const float* E, const float* A, float* dW, float* dbias, float* dE, float* ws,
                        int64_t M, int64_t L, int64_t D, int64_t V, int64_t F, int64_t KS, fn_stream_t stream);
int64_t fn_dta_pair_loss_ws(int64_t M);
int fn_dta_pair_fwd_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                        const float* target /*nullable*/, float* h, float* out, float* g /*nullable without target*/,
                        float* loss_part /*nullable without target*/, int64_t M, int64_t Kd, int64_t Kx, int64_t H, int64_t C,
                        fn_stream_t stream);
int fn_dta_pair_bwd_f32(const float* g, const float* drug, const float* xt, const float* h, const float* W1, const float* w2,
                        float* g_drug, float* g_xt, float* dW1, float* db1, float* dW2, float* db2, const float* loss_part /*nullable*/,
                        int64_t n_part, float* loss /*nullable*/, int64_t M, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream);
int fn_dta_pair_fwd_rows_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                             const float* target, float* h, float* out, float* g, float* loss_part, int64_t M, int64_t Kd, int64_t Kx,
                             int64_t H, int64_t C, const int32_t* real_rows /*nullable, device*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The pair head on a FACTORED batch; csrc/pair_factored.hip.  Entry points added under ABI 12 (nothing existing changes).  U distinct
 * drug rows drug[U,256], Cn distinct second rows second[Cn,K1] and the pair lists pair_drug[M], pair_second[M] (int64) stand for the M
 * duplicated rows of fn_*_pair_fwd_f32: out[m] = fc2(fc1(cat(drug[pair_drug[m]], second[pair_second[m]]))).  With W1 = [W1d | W1s]:
 *   fn_*_pair_factored_fwd_f32   A[U,H] = drug W1d^T and B[Cn,H] = second W1s^T (no bias; saved for the backward), alpha = A w2,
 *                          beta = B w2 (ws), out[m] = alpha[pair_drug[m]] + beta[pair_second[m]] + (b1 . w2 + b2) and, with a target,
 *                          g[m] = 2 (out[m] - target[m]) / M and loss_part[0] = mean((out - target)^2).  One launch behind a 4-byte
 *                          memset of the arrival counter in ws (fn_*_pair_factored_ws(U, Cn) floats).  M = 0: nothing is written.
 *   fn_*_pair_factored_bwd_f32   from g[M] and the pair orderings (per side rowptr[n + 1] and perm[M], int32: perm[rowptr[r] ..
 *                          rowptr[r + 1]) = the pairs of row r, ascending -- a stable sort of the pair list): g_drug[U,256] =
 *                          sd[u] v_d, g_second[Cn,K1] = ss[c] v_s (v = W1^T w2; sd, ss the sums of g over a row's pairs; the cdrp
 *                          instance zeroes g_second where second <= 0), dW1, db1, dW2, db2 and, with loss, loss[0] = the sum of
 *                          loss_part[n_part].  One launch.  A row no pair refers to gets exactly zero; M = 0 writes zeros everywhere.
 *   fn_*_pair_factored_grid_f32  out[U,Cn]: out[u,c] = the forward's value for the pair (u, c).  One launch, no backward.
 * Built for the widths of fn_cdrp_pair_* (K1 = 256, gated) and fn_dta_pair_* (K1 = 300, not gated) only: others FN_EUNSUPPORTED.  M, U,
 * Cn in [0, FN_DENSE_MAX_ROWS] (M > 0 needs U, Cn >= 1), else FN_EINVAL; both decided before anything is written.  No float atomics,
 * every sum in a fixed order: results are reproducible bit for bit.  A pair-list or ordering value is range-tested before it is used as
 * an index: a pair outside [0,U) x [0,Cn) gets out = 0, g = 0 and contributes to nothing.  drug, second, A, B, W1, g_drug, g_second,
 * dW1: 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int64_t fn_cdrp_pair_factored_ws(int64_t U, int64_t Cn);
int fn_cdrp_pair_factored_fwd_f32(const float* drug, const float* cell, const int64_t* pair_drug, const int64_t* pair_cell, const float* W1,
                                  const float* b1, const float* w2, const float* b2, const float* target /*nullable*/, float* A, float* B,
                                  float* ws, float* out, float* g /*nullable without target*/, float* loss_part /*nullable without target*/,
                                  int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream);
int fn_cdrp_pair_factored_bwd_f32(const float* g, const float* drug, const float* cell, const float* A, const float* B, const float* W1,
                                  const float* b1, const float* w2, const int32_t* rowptr_drug, const int32_t* perm_drug,
                                  const int32_t* rowptr_cell, const int32_t* perm_cell, float* g_drug, float* g_cell, float* dW1, float* db1,
                                  float* dW2, float* db2, const float* loss_part /*nullable*/, int64_t n_part, float* loss /*nullable*/,
                                  int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream);
int fn_cdrp_pair_factored_grid_f32(const float* drug, const float* cell, const float* W1, const float* b1, const float* w2, const float* b2,
                                   float* out, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc, int64_t H, int64_t C, fn_stream_t stream);
int64_t fn_dta_pair_factored_ws(int64_t U, int64_t Cn);
int fn_dta_pair_factored_fwd_f32(const float* drug, const float* xt, const int64_t* pair_drug, const int64_t* pair_prot, const float* W1,
                                 const float* b1, const float* w2, const float* b2, const float* target /*nullable*/, float* A, float* B,
                                 float* ws, float* out, float* g /*nullable without target*/, float* loss_part /*nullable without target*/,
                                 int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream);
int fn_dta_pair_factored_bwd_f32(const float* g, const float* drug, const float* xt, const float* A, const float* B, const float* W1,
                                 const float* b1, const float* w2, const int32_t* rowptr_drug, const int32_t* perm_drug,
                                 const int32_t* rowptr_prot, const int32_t* perm_prot, float* g_drug, float* g_xt, float* dW1, float* db1,
                                 float* dW2, float* db2, const float* loss_part /*nullable*/, int64_t n_part, float* loss /*nullable*/,
                                 int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream);
int fn_dta_pair_factored_grid_f32(const float* drug, const float* xt, const float* W1, const float* b1, const float* w2, const float* b2,
                                  float* out, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx, int64_t H, int64_t C, fn_stream_t stream);

/* fn_cdrp_pair_factored_fwd_rows_f32 / fn_dta_pair_factored_fwd_rows_f32 (added under ABI 12, nothing existing changes):
 * fn_*_pair_factored_fwd_f32 with a device-side count of the REAL pairs, for a step over static capacities (FN_STAGE_COUNT writes the
 * word).  n = *real_pairs clamped to [0, M]: pairs m < n get out, g[m] = 2 (out - target) / n and the loss partial is divided by n;
 * pairs m >= n get out = 0, g = 0 exactly and no share of the loss, and pair_drug / pair_second are not read there; n = 0: loss 0,
 * every g 0, nothing is divided.  real_pairs NULL: the plain entry point.  A count without a target, or a misaligned one: FN_EINVAL.
 * fn_*_pair_factored_bwd_f32 takes no count: with fn_pair_orderings_i32's orderings of the first n pairs a padding pair is in no
 * segment, a row no real pair refers to has a zero sum -- its g_drug / g_second row is exactly zero -- and adds 0 * x to dW1 and dW2
 * in the place of the sum it would have had, so every result equals, bit for bit, that of the plain calls on the real rows alone. */
int fn_cdrp_pair_factored_fwd_rows_f32(const float* drug, const float* cell, const int64_t* pair_drug, const int64_t* pair_cell, const float* W1,
                                       const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                       float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kc,
                                       int64_t H, int64_t C, const int32_t* real_pairs /*nullable, device*/, fn_stream_t stream);
int fn_dta_pair_factored_fwd_rows_f32(const float* drug, const float* xt, const int64_t* pair_drug, const int64_t* pair_prot, const float* W1,
                                      const float* b1, const float* w2, const float* b2, const float* target, float* A, float* B, float* ws,
                                      float* out, float* g, float* loss_part, int64_t M, int64_t U, int64_t Cn, int64_t Kd, int64_t Kx,
                                      int64_t H, int64_t C, const int32_t* real_pairs /*nullable, device*/, fn_stream_t stream);

/* fn_pair_orderings_i32 (added under ABI 12): the pair orderings of both sides of a factored batch, one launch, no host read, no
 * allocation, no atomic (a bitonic sort of distinct 24-bit keys in LDS): two runs give identical bits.  n = real_pairs ?
 * clamp(*real_pairs, 0, M) : M; only the first n pairs exist and what lies behind them in the lists is not read.  Per side (N = U for
 * pair_drug, Cn for pair_second): perm[rowptr[r] .. rowptr[r + 1]) = the pairs m < n whose value is r, ascending; a value outside
 * [0, N) -- compared as int64 -- belongs to no row; rowptr[N] = the number of in-range pairs; perm[rowptr[N] .. M) = -1.  M = 0 or
 * n = 0: all row pointers 0.  rowptr_*: [N + 1], perm_*: [M], int32.  M, U or Cn outside [0, FN_DENSE_MAX_ROWS]: FN_EINVAL. */
int fn_pair_orderings_i32(const int64_t* pair_drug, const int64_t* pair_second, const int32_t* real_pairs /*nullable, device*/,
                          int32_t* rowptr_drug, int32_t* perm_drug, int32_t* rowptr_second, int32_t* perm_second, int64_t M, int64_t U,
                          int64_t Cn, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Graph-convolution baseline, model_version gcn2 (reference model/gcn/gcn2.py:48-65); csrc/gcn.hip.  Entry points added under ABI 12
 * (nothing existing changes).  The aggregate is a degree-normalised neighbour sum over one of a level's two CSRs:
 *     y[i] = c[i] * sum over the items k of row i, in plan order, of c[nbr(k)] * x[nbr(k)]
 *   fn_gcn_coef_f32        c[i] = (extent of row i in the level's by-SOURCE CSR)^-1/2, 0 where the extent is 0: the reference's
 *                          degree(source) of the graph with self loops (the plan's loop items are counted), gcn2.py:51-53.  Once per
 *                          batch: the table is the same for every layer and both directions.
 *   fn_gcn_aggregate_f32   by_source = 0: rows are destinations, items the in-edges (rowptr_d, src_d, the loop item last) -- the forward;
 *                          by_source = 1: rows are sources, items the out-edges (rowptr_s, dst_s) -- the backward of the former, since
 *                          the weight c[s] c[t] is symmetric.  coef NULL: all ones (the fragment graph: gcn2.py:61-65).  out (nullable):
 *                          the raw rows; act (nullable, with act->y): y = relu?(dropout(raw)) on the Philox stream of fn_dropout_act_f32
 *                          over the [n,128] elements, so fn_dropout_act_bwd_f32 is its backward.  At least one of the two outputs.  A row
 *                          without items is written as zeros.  Items are added in plan order (ascending edge id), no atomics: results are
 *                          reproducible bit for bit.  x, out, y: [n,128], 16-byte aligned, x distinct from the outputs; n <= 2^23.
 * ------------------------------------------------------------------------------------------ */
int fn_gcn_coef_f32(const fn_gat_plan* plan, float* coef /*[n]*/, fn_stream_t stream);
int fn_gcn_aggregate_f32(const float* x, const fn_gat_plan* plan, int by_source, const float* coef /*nullable*/, float* out /*nullable*/,
                         const fn_act_epilogue* act /*nullable*/, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Nearest neighbours in embedding space; csrc/topk.hip.  Entry points added under ABI 12 (nothing existing changes).
 *   fn_rows_rnorm_f32   out[i] = 1 / max(|x_i|_2, 1e-12) of the rows of x [n, d]: one summation order per row (lane l of one wave adds
 *                       columns l, l + 64, .. in order, then a fixed butterfly), whatever n and the launch shape.
 *   fn_topk_update_f32  folds the library chunk lib [n_lib, d] into the running best lists of the queries q [n_q, d] (both fp32 row-major,
 *                       16-byte aligned; d = 128 or 256, else FN_EUNSUPPORTED).  k in [1, 32].  metric 0: the dot product, larger is
 *                       better; 1: cosine = dot * (q_aux[i] * lib_aux[j]) with the reciprocal norms passed in, larger is better; 2: squared
 *                       L2 = fma(-2, dot, q_aux[i] + lib_aux[j]) with the squared norms passed in, SMALLER is better.  index_base is the
 *                       global row id of lib[0]; exclude (nullable) [n_q] names the global id query i must skip, -1 for none.
 *                       best_score [n_q, k] / best_index [n_q, k] are read and written: sorted best first, empty slots index -1 and
 *                       score -inf (+inf for metric 2); a fresh state is all empty.  The order is total -- better score first, on equal
 *                       score the smaller global index -- and the dot of a pair is one fp32 fma chain over d in a fixed order (fp32-input
 *                       MFMA) wherever the row sits, so the lists are bit-identical however the library is cut into chunks and whatever
 *                       the launch shape (the chunks of one search must not overlap).  No atomics, no workgroup waits on another: a scan
 *                       launch leaves per-wave candidate lists in scratch, a merge launch folds them in.  Nothing of size n_q x n_lib
 *                       exists.  splits: 0 = the library's own choice of slices per chunk, 1..63 = that many (a test's handle on the
 *                       launch shape; fewer when the chunk has fewer 16-row tiles).  scratch: 16-byte aligned device bytes, at least
 *                       fn_topk_scratch_bytes(t) (which reads n_q, n_lib, k and splits only; FN_EINVAL, negative, when they are invalid).
 *                       n_lib = 0 or n_q = 0: nothing is launched.  A null pointer, a negative size, k outside [1, 32], a metric outside
 *                       0..2 or too small a scratch: FN_EINVAL.  The order of NaN scores is undefined.
 * ------------------------------------------------------------------------------------------ */
typedef struct fn_topk {
    const float *q /*[n_q,d]*/, *lib /*[n_lib,d]*/, *q_aux /*[n_q], metric 1, 2*/, *lib_aux /*[n_lib], metric 1, 2*/;
    const int64_t* exclude;      /* [n_q], nullable */
    float* best_score;           /* [n_q,k] */
    int64_t* best_index;         /* [n_q,k] */
    void* scratch;
    int64_t scratch_bytes, n_q, n_lib, index_base;
    int32_t d, k, metric, splits;
} fn_topk;
int fn_rows_rnorm_f32(const float* x /*[n,d]*/, int64_t n, int64_t d, float* out /*[n]*/, fn_stream_t stream);
int64_t fn_topk_scratch_bytes(const fn_topk* t);
int fn_topk_update_f32(const fn_topk* t, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metrics on the device; csrc/metrics.hip.  Entry points added under ABI 12 (nothing existing changes).
 * Both read pred [n, c] and label [n, c] (fp32, row-major, contiguous, 4-byte aligned) and treat every column on its own.  Row i is
 * VALID in column k iff label[i,k] >= label_floor (a NaN label is never valid): -0.5 is the "missing label" convention of the
 * classification targets, -inf takes every non-NaN label.  c in [1, FN_METRICS_MAX_COLS], n <= 2^24.
 *   fn_pair_concordance_f32  out [c][FN_CONC_FIELDS] uint64, per column: n_valid; n_nan = valid rows whose prediction is NaN (they take
 *                       part in no pair); n_pairs = ORDERED pairs (i, j) of valid, non-NaN rows with label_i > label_j; n_conc = those
 *                       with pred_i > pred_j; n_tied = those with pred_i == pred_j.  Plain IEEE compares on the fp32 values (-0 == 0,
 *                       +inf == +inf is a tie).  (n_conc + n_tied / 2) / n_pairs is the concordance index; on binary labels, ROC-AUC.
 *                       The counts are exact integers, so they are the same for every launch shape and every run.  A count launch
 *                       (workgroup = FN_CONC_TILE i-rows x one slice of FN_CONC_TILE-row j-tiles of one column; the j-tile in LDS, four
 *                       i-rows per lane in registers) leaves one row per workgroup in scratch, a second launch adds them per column: no
 *                       atomics, no memset.  splits: 0 = the library's choice of j-slices, else that many (fewer when there are fewer
 *                       j-tiles) -- a test's handle on the tile boundaries.  Cost O(n^2 c).
 *   fn_regression_sums_f32   out [c][FN_SUMS_FIELDS] double, per column over the valid rows, with p = pred * scale + shift (an fp32
 *                       multiply, then an fp32 add: never one fma) and y = label: n, sum y, sum p, sum y^2, sum p^2, sum y p,
 *                       sum (y - p)^2, sum |y - p|, every term formed and added in fp64.  ONE order of addition: rows are cut into
 *                       chunks of FN_SUMS_CHUNK; inside a chunk thread t of 256 adds rows t, t + 256, .., then a fixed butterfly and the
 *                       four wave sums in order; the chunk rows of a column are added by a second launch the same way.  The order depends
 *                       on n alone, so results are bit-identical across runs and across splits (0 = the library's choice of workgroups
 *                       per column, else that many; each walks chunks splits apart).
 * scratch: 8-byte aligned device bytes, at least fn_metrics_scratch_bytes(m, sums) (reads n, c and splits only; FN_EINVAL, negative,
 * when they are invalid).  n = 0: nothing is launched but one fill of zeros (pred, label and scratch may be null).  A null pointer, a negative size, n > 2^24, c outside
 * [1, FN_METRICS_MAX_COLS], a negative splits or too small a scratch: FN_EINVAL, and the GPU is not touched.
 * ------------------------------------------------------------------------------------------ */
#define FN_METRICS_MAX_COLS 64
#define FN_CONC_FIELDS 5
#define FN_CONC_TILE 512
#define FN_SUMS_FIELDS 8
#define FN_SUMS_CHUNK 1024
typedef struct fn_metrics {
    const float *pred /*[n,c]*/, *label /*[n,c]*/;
    void* out;                   /* [c][FN_CONC_FIELDS] uint64 / [c][FN_SUMS_FIELDS] double */
    void* scratch;
    int64_t scratch_bytes, n;
    float label_floor, scale, shift;     /* scale, shift: fn_regression_sums_f32 only */
    int32_t c, splits;
} fn_metrics;
int64_t fn_metrics_scratch_bytes(const fn_metrics* m, int sums);
int fn_pair_concordance_f32(const fn_metrics* m, fn_stream_t stream);
int fn_regression_sums_f32(const fn_metrics* m, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Diverse subsets of embedding rows: greedy k-centre (Gonzalez; farthest-point / MaxMin picking); csrc/kcenter.hip.  Entry points
 * added under ABI 12 (nothing existing changes).  The run's state is the caller's: mind [n] (distance of every row to its nearest
 * centre so far; fill +inf -- or a distance to something else, every value >= +0 or NaN -- before the first centre), label [n] (ordinal
 * of that centre; fill -1), picked [cap], radius [cap + 1], count [1] (centres folded in so far, seeds and picks; fill 0).
 *   Distances.  metric 0: squared L2 in its direct form, sum_j (x_ij - c_j)^2 as an fma(diff, diff, acc) chain (never
 *                       |x|^2 + |c|^2 - 2 x.c: nothing cancels, a row is at distance exactly 0 of itself).  metric 1: the cosine
 *                       distance max(0, 1 - dot * (aux_i * aux_c)), aux = fn_rows_rnorm_f32 of the rows.  The additions of one row have
 *                       ONE order (lane l of the row's lanes adds its columns 4 l .. 4 l + 3 in order, then a fixed butterfly) whatever
 *                       n, the grid, splits or the call a pass belongs to: mind, label, picked and radius are bit-identical for every
 *                       launch shape, and for pick(a) then pick(b) against pick(a + b).
 *   Update rule.        For a new centre of ordinal t: if (dist < mind[i]) { mind[i] = dist; label[i] = t; } -- strict, the earlier
 *                       centre keeps a tie.  A NaN distance lowers nothing.
 *   Pick rule.          A total order: the unpicked row with the largest mind, on equal mind the smallest row.  A NaN mind never wins
 *                       while a number is left; among NaNs the smallest row.  A row is picked at most once: the picked row's mind is
 *                       stored as -0.0f (distance zero; the sign bit is the mark, and the only state besides the arrays above).
 *                       Duplicates of a picked row have mind +0 and may be picked later.
 *   radius.             radius[t] = mind of the row picked as ordinal t, read when it was picked: the coverage radius of the centres
 *                       before it (+inf for the first centre of an unseeded run).  When a pick call returns, radius[count] holds the
 *                       largest remaining mind, the coverage radius of everything chosen (0 when no row is left).  A seed's slot
 *                       holds picked -1 and radius NaN.
 *   fn_kcenter_pick_f32 k picks.  first: the row of the very first centre, or -1 = the arg-max like every later pick.  One launch per
 *                       pick (each reduces the <= 512 per-workgroup (mind, row) pairs of the launch before it, folds the winner in and
 *                       leaves its own pairs), one scan launch in front when first is -1, one closing launch; no atomics, no workgroup
 *                       waits on another, nothing synchronises with the host.
 *   fn_kcenter_seed_f32 folds s given centres [s, d] in (centres_aux [s]: their fn_rows_rnorm_f32, metric 1): one update launch each, no
 *                       pick, ordinals count .. count + s - 1.  For seed sets of up to a few thousand rows; a distance to a larger set
 *                       goes in through mind.
 * host_count / host_picks: what the caller knows *count and the number of picked rows to be (the library does not read device memory);
 * splits: 0 = the library's choice of workgroups, 1..512 = at most that many (a test's handle on the launch shape).  scratch: 16-byte
 * aligned device bytes, at least fn_kcenter_scratch_bytes(k); it carries nothing from call to call.  n = 0 or k = 0: nothing is
 * launched.  A null pointer, a negative size, k > n - host_picks, host_count + k (or + s) > cap, first outside [-1, n), first >= 0 with
 * host_count > 0, a metric outside 0..1 or too small a scratch: FN_EINVAL; d other than 128 or 256: FN_EUNSUPPORTED; the GPU is not
 * touched.  Whatever the host says, a launch records nothing at or behind cap and picks nothing when no row is left.
 * ------------------------------------------------------------------------------------------ */
typedef struct fn_kcenter {
    const float* x;              /* [n,d] fp32 row-major, 16-byte aligned */
    const float* aux;            /* [n], metric 1; else nullable */
    float* mind;                 /* [n] in/out */
    int32_t* label;              /* [n] in/out */
    int64_t* picked;             /* [cap] out: rows in pick order, by ordinal */
    float* radius;               /* [cap + 1] out */
    int64_t* count;              /* [1] device word, in/out */
    void* scratch;
    int64_t scratch_bytes, n, cap, host_count, host_picks;
    int32_t d, metric, splits;
} fn_kcenter;
int64_t fn_kcenter_scratch_bytes(const fn_kcenter* k);
int fn_kcenter_seed_f32(const fn_kcenter* k, const float* centres /*[s,d]*/, const float* centres_aux /*[s], nullable*/, int64_t s,
                        fn_stream_t stream);
int fn_kcenter_pick_f32(const fn_kcenter* k, int64_t first, int64_t n_picks, fn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Moments and projections of a row table (the chemical-space map and the Mahalanobis domain); csrc/moments.hip.  Entry points added
 * under ABI 12 (nothing existing changes).  x [n, d] fp32 row-major, 16-byte aligned, d = 128 or 256 (else FN_EUNSUPPORTED); shift [d]
 * fp32, nullable = zeros; z = x - shift is ONE fp32 subtraction per element.
 *   fn_rows_moments_f32 sum [d] double, sum[j] = sum_i z_ij; gram [d, d] double, gram[j][l] = sum_i z_ij z_il.  accumulate != 0: the
 *                       call's result is added onto what sum / gram hold, one fp64 addition per entry (a store arrives batch by
 *                       batch); else they are overwritten.  ONE order of addition, a function of n alone: the rows of a call are cut
 *                       into chunks of FN_MOMENTS_CHUNK rows counted from the call's row 0; inside a chunk a Gram entry is one fp32 fma
 *                       chain over the chunk's rows in ascending order (the fp32-input MFMA 16x16x4 is bit for bit such a chain), a
 *                       column sum four fp32 chains of adds (rows = 0, 1, 2, 3 mod 4); the chunk results of a SUPER-CHUNK
 *                       (FN_MOMENTS_GROUP consecutive chunks) are added in fp64 in ascending order by the one workgroup that owns that
 *                       super-chunk's 64 x 64 block of the Gram matrix (the four partial column sums of a super-chunk then in the order
 *                       ((0 + 1) + 2) + 3), and a second launch adds the super-chunk results in ascending order.  No atomics, no
 *                       workgroup waits on another.  Only the blocks on and above the diagonal are computed; gram[l][j] is a copy of
 *                       gram[j][l].  The result is a function of (x, shift, n, d): bit-identical for every launch shape.  It is NOT
 *                       promised to be bit-identical when the same rows arrive cut into different calls: chunks are counted per call.
 *                       splits: 0 = the library's choice of workgroups, else at most that many (a test's handle on the launch shape).
 *                       scratch: 16-byte aligned device bytes, at least fn_moments_scratch_bytes(m) =
 *                       ceil(n / (FN_MOMENTS_CHUNK * FN_MOMENTS_GROUP)) * (d * d + d) doubles -- one slot per super-chunk, not per
 *                       chunk: 32 768 rows a slot, so 1 M rows of 256 floats take 32 slots = 16.8 MB (of 128: 4.2 MB).  n = 0: sum and
 *                       gram are left alone (accumulate) or zeroed; x and scratch may be null.  Rows past n are never read.
 *   fn_rows_project_f32 W [d, k] fp32 row-major, 4-byte aligned, 1 <= k <= d.  out [n, k] fp32 (nullable), out[i][c] = one fp32 fma
 *                       chain, started at 0, of z_ip W_pc over p in the order p = 16 t + 4 h + e for t = 0 .. d/16 - 1 (outer),
 *                       e = 0 .. 3, h = 0 .. 3 (inner) -- the same permutation for every row and column.  sq [n] fp32 (nullable; one of
 *                       the two must be given), sq[i] = one fp32 fma chain over c ascending of out[i][c]^2, started at 0.  Row i's
 *                       results depend on row i, shift and W alone: a slice of the rows gives the same bits as the whole table,
 *                       whatever the launch shape.  With out null no n x k table exists anywhere.
 * A null descriptor or required pointer, a negative size or splits, n >= 2^40, k outside [1, d], a misaligned buffer or too small a
 * scratch: FN_EINVAL, and the GPU is not touched.
 * ------------------------------------------------------------------------------------------ */
#define FN_MOMENTS_CHUNK 512       /* rows of one fp32 chain; a multiple of 64, <= 1024 */
#define FN_MOMENTS_GROUP 64        /* chunks of one super-chunk = one scratch slot */
typedef struct fn_moments {
    const float* x;              /* [n,d] */
    const float* shift;          /* [d], nullable */
    double* sum;                 /* [d] */
    double* gram;                /* [d,d] */
    void* scratch;
    int64_t scratch_bytes, n;
    int32_t d, accumulate, splits;
} fn_moments;
typedef struct fn_project {
    const float* x;              /* [n,d] */
    const float* shift;          /* [d], nullable */
    const float* W;              /* [d,k] */
    float* out;                  /* [n,k], nullable */
    float* sq;                   /* [n], nullable */
    int64_t n;
    int32_t d, k;
} fn_project;
int64_t fn_moments_scratch_bytes(const fn_moments* m);
int fn_rows_moments_f32(const fn_moments* m, fn_stream_t stream);
int fn_rows_project_f32(const fn_project* p, fn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FRAGNET_HIP_H */
