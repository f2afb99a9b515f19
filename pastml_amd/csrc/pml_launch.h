// What pml_api.hip (schedules, C-ABI) and pml_api_readers.hip call of the kernel launchers, which live in translation units of their own
// (pml_launch_*.hip, one per kernel family, compiled in parallel): the dispatch functions, the cases of lane shapes they are
// instantiated for (the shapes themselves: pml_columns.h) and the predicates that say which family a context's sweeps take.
#pragma once
#include <type_traits>
#include "pml_host.h"
#include "pml_time_segments.h"

// ---------------------------------------------------------------------------------------------------------------------
// (G, R) dispatch
// ---------------------------------------------------------------------------------------------------------------------
#define PML_GR_CASES(X)  \
    X(8, 4)              \
    X(1, 1)              \
    X(2, 1)              \
    X(4, 1)              \
    X(8, 1)              \
    X(16, 1)             \
    X(64, 1)             \
    X(32, 2)             \
    X(64, 2)             \
    X(64, 4)


#define PML_F81_CASES(X) \
    X(2, 2)              \
    X(4, 2)              \
    X(1, 1)              \
    X(1, 2)              \
    X(1, 4)              \
    X(2, 4)              \
    X(4, 4)              \
    X(8, 4)              \
    X(16, 4)             \
    X(32, 4)             \
    X(64, 4)             \
    X(32, 2)             \
    X(16, 2)             \
    X(8, 8)


#define PML_SUPER_CASES(X) \
    X(8, 4)                \
    X(16, 4)               \
    X(8, 8)

// Two-level units run in the lane shape the level kernels give the levels they replace where those do not stream stored
// vectors (PmlColumnPlan::bu_shape) -- units of 8 lanes and more, single-word masks.
static bool super_units(const pml_ctx* ctx) {
    if (!ctx->sup.ok || ctx->kind != PML_MODEL_F81 || ctx->W != 1) return false;
    for (const PmlLaneShape s : {ctx->cols.bu_shape(), ctx->cols.td_shape()})
        if (s.g < 8 || (s.g == 16 && s.r == 2)) return false;   // (16 x 2: the shape of forests with polytomies, no two-level kernels)
    return true;
}

// the sweeps of this context run the level schedule with two-level units (not one launch per sweep, not subtree blocks)
static bool super_sweeps(const pml_ctx* ctx) {
    return super_units(ctx) && !single_launch_sweeps(ctx) && !block_schedule(ctx);
}

// the thin ends of a large forest as subtree blocks (pml_tree_upload).  Measured, marginal pass, default against NO_THIN
// (profiles/r05u_thin_ends.txt): 100 000 tips with polytomies x 16 characters k = 4 1.43 -> 1.16 ms, k = 20 1.79 -> 1.55;
// random binary 40 000 tips x 8 k = 4 0.368 -> 0.313, k = 64 0.587 -> 0.504; 262 144 tips x 32 k = 4 1.60 -> 1.54,
// k = 12 2.54 -> 2.49, k = 20 3.50 -> 3.43 (there the wide levels dominate).  NO_THIN_WIDE: units of fewer than 8 lanes only.
static bool thin_bottom_up(const pml_ctx* ctx) {
    return ctx->thin.ok && ctx->kind == PML_MODEL_F81 && !ctx->tune.on(T_NO_THIN) &&
           (ctx->cols.bu_shape().g < 8 || !ctx->tune.on(T_NO_THIN_WIDE));
}
static bool deep_top_down(const pml_ctx* ctx) {
    return ctx->deep.ok && ctx->kind == PML_MODEL_F81 && !ctx->tune.on(T_NO_THIN) && (ctx->cols.Gt < 8 || !ctx->tune.on(T_NO_THIN_WIDE));
}


// sum sweeps of the eigen models without forming P(t) (pml_kernels_eigen_gemm.h): one launch over a list (nodes) or a
// contiguous id range (first) of n nodes
// (any eigen model with up to 64 states; 65 - 128 states: the reversible ones -- pml_model_set_eigen checks what it is given --,
// whose A^-1 is A transposed and rescaled, so that one matrix in LDS serves both products)
static bool eigen_gemm(const pml_ctx* c) {
    const bool off = c->tune.on(T_NO_EIGEN_GEMM) || c->tune.on(T_NO_MFMA) || c->tune.on(T_NO_EIGEN_FUSED);
    if (off || !c->eig_fused_opt || c->kind != PML_MODEL_EIGEN || c->k < 2) return false;
    if (c->k <= 64) return c->W == 1;
    return c->k <= 128 && c->W == 2 && c->eig_sym_all && c->d_Asym != nullptr;
}


// The joint sweep of the eigen models on the vector units (pml_kernels_eigen_joint.h) for 2 <= k <= 64;
// PASTML_HIP_NO_EIGEN_JOINT_VALU keeps the matrix-core kernels (pml_kernels_eigen_mfma.h).
static bool eigen_joint_valu(const pml_ctx* c) {
    const bool off = c->tune.on(T_NO_EIGEN_JOINT_VALU);
    return !off && c->eigj_valu_opt && c->kind == PML_MODEL_EIGEN && c->k >= 2 && c->k <= 64 && c->W == 1 &&
           c->d_AinvT != nullptr;
}


// ---- pml_launch_matrix.hip: sweeps of the models with a materialised (or closed-form 4 x 4) P(t), state selection
//      window: -1, or which of the context's slot tables (0 bottom-up, 1 top-down) locates P(t) of the launch's children in the
//      window (pml_pij_window.h)
PML_INTERNAL int dispatch_sweep_matrix(pml_ctx* ctx, SweepKind what, const int* level, int n_level, int window = -1);
PML_INTERNAL int dispatch_select(pml_ctx* ctx, int method, int force_joint, const u64* d_lh_mask);
// ---- pml_launch_f81_level.hip: F81-family level launches over n_level units.  cherries: the top-down staging hint (some unit
//      has a cherry among its first two children); bu_sweep: part of a bottom-up sweep, which looks at the active-column flags
PML_INTERNAL int dispatch_sweep_f81(pml_ctx* ctx, SweepKind what, const PmlUnit* units, int n_level, bool cherries, bool bu_sweep);
// ---- pml_launch_f81_wide.hip: the same for more than 256 states (64 lanes x 8 states)
PML_INTERNAL int dispatch_sweep_f81_wide(pml_ctx* ctx, SweepKind what, const PmlUnit* units, int n_level, bool cherries, bool bu_sweep);
// ---- pml_launch_f81_small.hip / pml_launch_f81_blocks.hip: several levels in one launch (whole sweeps of small forests and
//      the narrow ends; subtree blocks and the thin ends).  signal: the launch raises the completion word
PML_INTERNAL int dispatch_small_f81(pml_ctx* ctx, bool bottom_up, bool signal, int do_prep, int first_level, int n_levels,
                                    const PmlUnit* units = nullptr, const int* d_offsets = nullptr, int skip_roots = 0);
PML_INTERNAL int dispatch_blocks_f81(pml_ctx* ctx, bool bottom_up, int which, bool signal);
// ---- pml_launch_f81_super.hip: two-level and stacked units
//      chain >= 0: the launch also runs the stacked units of that depth (top-down, td_f81_chain_kernel) or of that level
//      (bottom-up, bu_f81_chain_kernel)
PML_INTERNAL int dispatch_super_f81(pml_ctx* ctx, bool bottom_up, int chain = -1);
PML_INTERNAL int dispatch_stack_f81(pml_ctx* ctx, bool bottom_up, int level);
// ---- pml_launch_eigen_mfma.hip: fused FP64 matrix-core sweeps of the eigen models, P(t) batch on the matrix cores
PML_INTERNAL int launch_eigen_fused(pml_ctx* ctx, int mode, const int* nodes, int first, int n, int tips);
PML_INTERNAL int launch_eigen_narrow(pml_ctx* ctx, int mode, const int* nodes, const int* d_offsets, int first_level, int n_levels);
PML_INTERNAL int launch_eigen_tips(pml_ctx* ctx, int joint);
PML_INTERNAL int launch_pij_mfma(pml_ctx* ctx);
PML_INTERNAL int launch_pij_wide(pml_ctx* ctx);
//      the list form: P(t) of `count` branches of a device list into the slots 0 .. count - 1 of the window of B slots per column;
//      arm_pij_wide_list asks for the kernel's LDS once, outside any stream capture (pml_pij_window_set)
//      for the columns [col_begin, col_end) of the context only (col_end < 0: all of them), whose windows are the first
//      col_end - col_begin of the buffer: a call for one column does not pay for the others
PML_INTERNAL int launch_pij_wide_list(pml_ctx* ctx, double* window, long long B, const int* d_branches, int count, int col_begin = 0,
                                      int col_end = -1);
PML_INTERNAL int arm_pij_wide_list(pml_ctx* ctx);
// ---- pml_launch_eigen_gemm.hip: sum sweeps as two small GEMMs per 16 nodes
PML_INTERNAL int launch_eigen_gemm(pml_ctx* ctx, int mode, const int* nodes, int first, int n);
PML_INTERNAL int launch_eigen_gemm_narrow(pml_ctx* ctx, int mode, const int* nodes, const int* d_offsets, int first_level,
                                          int n_levels, const int* d_blk_start = nullptr, int n_blocks = 1);
// ---- pml_launch_eigen_gemm_wide.hip: the same for 65 - 128 states (one matrix in LDS)
PML_INTERNAL int launch_eigen_gemm_wide(pml_ctx* ctx, int mode, const int* nodes, int first, int n);
PML_INTERNAL int launch_eigen_gemm_narrow_wide(pml_ctx* ctx, int mode, const int* nodes, const int* d_offsets, int first_level,
                                               int n_levels, const int* d_blk_start, int n_blocks);
// ---- pml_launch_eigen_joint.hip: joint sweep of the eigen models on the vector units, P(t) batch for k < 16
PML_INTERNAL int launch_eigen_joint(pml_ctx* ctx, const PmlUnit* units, const int* d_offsets, int first, int n,
                                    const int* d_blk_start = nullptr, int n_blocks = 1);
PML_INTERNAL int launch_eigen_joint_tips(pml_ctx* ctx);
PML_INTERNAL int launch_pij_valu(pml_ctx* ctx);
// ---- pml_launch_simulate.hip: forward simulation of a column along the forest (pml_simulate_states); d_states [N][rs] in the
//      caller's numbering, uint8 for k <= 256, else uint16
PML_INTERNAL int launch_simulate(pml_ctx* ctx, int col, int rep_offset, u64 seed, void* d_states, size_t rs);
//      its schedule, which the scenario sampler shares: the frontier depth D for n_tiles repetition tiles per node, and the preorder
//      lists of the subtrees rooted at depth D (ctx->d_sim_lists / d_sim_off / sim_n_lists)
PML_INTERNAL int sim_frontier_depth(const pml_ctx* ctx, int n_tiles);
PML_INTERNAL int sim_subtree_lists(pml_ctx* ctx, int D);
//      On a context with a P(t) window (pml_pij_window.h) the two run the windowed form of that schedule: the levels above the
//      frontier and the frontier's subtrees cut into runs of at most B branches (pml_plan_sim_window), each behind the launch that
//      builds the run's matrices for the call's column.  sim_window_prepare plans and uploads it into the call's scope -- `w` is
//      declared before the scope, whose copies read its host tables --, sim_window_run issues it (launch(args): one launch).
static inline bool pij_windowed(const pml_ctx* ctx) {
    return ctx->pij_window > 0 && ctx->kind == PML_MODEL_EIGEN && ctx->d_pij_window != nullptr;
}
struct SimWindowDevice {
    PmlSimWindowPlan plan;
    std::vector<int4> lists;   // entries of the frontier subtrees (PmlSimArgs::lists), the slot in the fourth field
    int* d_order = nullptr;    // plan.order
    int4* d_lists = nullptr;
    int* d_off = nullptr;      // plan.sub_off
};
PML_INTERNAL int sim_window_prepare(pml_ctx* ctx, int D, CallScope& mem, SimWindowDevice& w);
template <class Args, class Launch>
static inline int sim_window_run(pml_ctx* ctx, Args a, const SimWindowDevice& w, int col, const Launch& launch) {
    for (int part = 0; part < 2; ++part)
        for (const PmlSimWindowRun& r : part == 0 ? w.plan.levels : w.plan.groups) {
            if (r.build_count > 0)
                PML_TRY(launch_pij_wide_list(ctx, ctx->d_pij_window, ctx->pij_window, w.d_order + r.build_first, r.build_count, col, col + 1));
            a.lists = part == 0 ? nullptr : w.d_lists;
            a.list_off = part == 0 ? nullptr : w.d_off + r.first;
            a.first_node = part == 0 ? r.first : 0;
            a.n_lists = r.count;
            PML_TRY(launch(a));
        }
    return PML_OK;
}
// ---- pml_launch_scenarios.hip: scenarios of a column from the joint posterior after a marginal pass (pml_sample_scenarios);
//      d_states as for launch_simulate, d_fallback: one counter (zeroed)
PML_INTERNAL int launch_scenarios(pml_ctx* ctx, int col, int n_rep, int rep_offset, u64 seed, void* d_states, size_t rs,
                                  unsigned long long* d_fallback);
// ---- pml_launch_parsimony.hip: the parsimony passes on packed state sets (pml_parsimony); host arrays in the caller's numbering
PML_INTERNAL int launch_parsimony(pml_ctx* ctx, int n_cols, int k, const u64* given, int methods, u64* sets_out, i64* steps_out,
                                  i64* hist_out);
// ---- pml_launch_compress.hip: vertical collapse of the forest by equal state sets (pml_compress_vertical); host arrays in the
//      caller's numbering
PML_INTERNAL int launch_compress(pml_ctx* ctx, int n_cols, int W, const u64* sets, const unsigned char* is_polytomy, int* top_out,
                                 int* tips_out, int* internal_out, int* parent_vertex_out);
// ---- pml_launch_compress_horizontal.hip: one pass of the horizontal merging over a forest of V vertices
//      (pml_compress_horizontal); host arrays, rows of the vertex forest
#define PML_HZ_SORT_TILE 1024   // children of one vertex that a workgroup sorts in LDS (pml_compress_horizontal_info reports it)
PML_INTERNAL int launch_compress_horizontal(pml_ctx* ctx, int V, int n_cols, int W, const int* parent, const int* rank, const int* bin,
                                            const int* width_in, const unsigned char* live_in, const u64* sets, int* into_out,
                                            unsigned char* live_out, int* width_out, int* groups_out);
// ---- pml_launch_compress_trim.hip: the trimming of a horizontally merged forest of L live vertices in pre-order
//      (pml_compress_trim); host arrays, entries of the vertex forest
#define PML_TRIM_SCAN_TILE 1024   // entries of one workgroup of the prefix count (pml_compress_trim_info reports it)
PML_INTERNAL int launch_compress_trim(pml_ctx* ctx, int L, int n_cols, int W, const int* parent, const int* tree, const int* T,
                                      const int* w, const u64* sets, int tip_size_threshold, int n_trees,
                                      const unsigned char* trim_tree, double* tsize_out, unsigned char* keep_out,
                                      unsigned char* spliced_out, int* new_parent_out, unsigned char* moved_out, double* threshold_out);
// ---- pml_launch_timeline.hip: dates, get_date and the per-milestone counts of the compressed map (pml_timeline); host arrays
#define PML_TL_FUSE_WIDTH 512   // levels of at most this many nodes may share a launch of one workgroup (pml_timeline_info reports it)
PML_INTERNAL int launch_timeline(pml_ctx* ctx, const pml_timeline_in& in, const pml_timeline_out& out);

// ---- pml_launch_counts.hip: n_rep sampled scenarios of column col counted per node and per transition (pml_marginal_counts);
//      d_alt [N] in the library's numbering or null, d_counts [N][k], d_result [k][k] (zeroed), d_same [N][k] (zeroed) or null, all
//      in the caller's numbering; queued only.  counts_max_states: the most states its kernels hold
PML_INTERNAL int counts_max_states();
PML_INTERNAL int launch_counts(pml_ctx* ctx, int col, int n_rep, u64 seed, const unsigned char* d_alt, int* d_counts, long long* d_result,
                               int* d_same);
// ---- pml_launch_expected.hip: exact expected transition counts of the columns [cb, ce) (pml_expected_counts); d_alt [N] in the
//      library's numbering or null, d_out [cols][k][k], d_same [cols][N][k] in the caller's numbering (zeroed) or null
PML_INTERNAL int launch_expected(pml_ctx* ctx, int cb, int ce, const unsigned char* d_alt, double* d_out, double* d_same);
// ---- pml_launch_gradient.hip: exact gradient of ln L of the F81 family for the columns [cb, ce) (pml_loglik_gradient); device
//      arrays d_rates [cols][3], d_pi [cols][k], d_flat [cols]; queued only: the partials go into the caller's scope, which waits
PML_INTERNAL int launch_gradient(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_rates, double* d_pi, int* d_flat);
//      The lane shape <G, R> of the passes that stream v_n and q_p once per branch (the gradient here, the two exact histories
//      of the F81 family below) at k <= 512 states: f(G, R), the two as std::integral_constant
template <class F>
static inline void with_branch_shape(int k, const F& f) {
    using std::integral_constant;
    if (k <= 4) f(integral_constant<int, 1>{}, integral_constant<int, 4>{});
    else if (k <= 16) f(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    else if (k <= 64) f(integral_constant<int, 16>{}, integral_constant<int, 4>{});
    else if (k <= 256) f(integral_constant<int, 64>{}, integral_constant<int, 4>{});
    else f(integral_constant<int, 64>{}, integral_constant<int, 8>{});
}
// ---- pml_launch_history.hip: exact expected dwell times and Markov jumps of the F81 family for the columns [cb, ce)
//      (pml_expected_history); device arrays d_times [cols][k], d_jumps [cols][k][k] or null, d_branch [cols][N] in the caller's
//      numbering or null; queued only: partials and staged scalars go into the caller's scope, which waits
//      history_piece / history_jump_piece: ids (per time interval: segments) per piece of the branch pass and of the jump product;
//      history_args: the fields of a that come from the context and from cb, everything else zeroed
struct PmlHistArgs;
PML_INTERNAL int history_piece(int k);
PML_INTERNAL int history_jump_piece(int k);
PML_INTERNAL void history_args(const pml_ctx* ctx, int cb, PmlHistArgs& a);
PML_INTERNAL int launch_history(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_times, double* d_jumps, double* d_branch);
// ---- pml_launch_history_eigen.hip: the same for the eigen-decomposed models, 2 <= k <= 256 (pml_expected_history_eigen); the
//      same device arrays; queued only: the staged vectors and the partials go into the caller's scope, which waits
//      heig_rows: the values of c a lane of the pair sum keeps in registers at k states; with_heig_rows: f(CR), CR =
//      heig_rows(k) as a std::integral_constant
//      heig_args: the fields of a that come from the context and from cb, tc and td, everything else zeroed; launch_heig_basis:
//      the changes of basis per branch into a.stage and a.tprime, which both entries of the eigen models begin with
struct PmlHeigArgs;
PML_INTERNAL int heig_rows(int k);
template <class F>
static inline void with_heig_rows(int k, const F& f) {
    using std::integral_constant;
    const int CR = heig_rows(k);
    if (CR == 4) f(integral_constant<int, 4>{});
    else if (CR == 16) f(integral_constant<int, 16>{});
    else if (CR == 32) f(integral_constant<int, 32>{});
    else f(integral_constant<int, 64>{});
}
PML_INTERNAL void heig_args(const pml_ctx* ctx, int cb, PmlHeigArgs& a);
PML_INTERNAL void launch_heig_basis(pml_ctx* ctx, int cols, const PmlHeigArgs& a);
PML_INTERNAL int launch_history_eigen(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_times, double* d_jumps, double* d_branch);
// ---- pml_launch_history_sample.hip: histories of column col drawn on the scenarios d_states [N][rs] that launch_scenarios left
//      on the device (pml_sample_histories); device arrays d_times [n_rep][k], d_jumps [n_rep][k][k] (zeroed) or null, d_branch
//      [N][n_rep] in the caller's numbering or null, d_skipped: one counter (zeroed); queued only: the partials go into the
//      caller's scope, which waits
PML_INTERNAL int launch_history_sample(pml_ctx* ctx, CallScope& mem, int col, int n_rep, int rep_offset, u64 seed, const void* d_states,
                                       size_t rs, double* d_times, unsigned* d_jumps, unsigned short* d_branch,
                                       unsigned long long* d_skipped);
// ---- pml_launch_history_time.hip: the same per time interval, with the lineages at every boundary (pml_history_through_time).
//      plan: the segments (pml_time_segments.h); pieces / jpieces: its cut by history_piece(k) with the pseudo-bin and by
//      history_jump_piece(k) without -- all three the caller's, alive until its scope has waited.  Device arrays d_times
//      [cols][M][k], d_jumps [cols][M][k][k] or null, d_lineages [cols][M + 1][k] or null; queued only
PML_INTERNAL int launch_history_time(pml_ctx* ctx, CallScope& mem, int cb, int ce, const PmlTimeSegments& plan, const PmlTimePieces& pieces,
                                     const PmlTimePieces& jpieces, double* d_times, double* d_jumps, double* d_lineages);
// ---- pml_launch_history_time_eigen.hip: launch_history_time for the eigen-decomposed models, 2 <= k <= 256
//      (pml_history_through_time_eigen).  host: the caller's -- plan filled in, the rest derived from it by
//      history_time_eigen_plan --, alive until the caller's scope has waited.  The same device arrays; queued only
struct HistoryTimeEigenPlan {
    PmlTimeSegments plan, flagged;   // all segments; those that add to the lineages of a boundary, as a plan of their own
    PmlTimePieces pieces, lpieces;   // of plan without the pseudo-bin; of flagged with it
};
PML_INTERNAL void history_time_eigen_plan(HistoryTimeEigenPlan& host);
PML_INTERNAL int launch_history_time_eigen(pml_ctx* ctx, CallScope& mem, int cb, int ce, const HistoryTimeEigenPlan& host,
                                           double* d_times, double* d_jumps, double* d_lineages);
// ---- pml_launch_history_time_sample.hip: the histories of launch_history_sample cut at the boundaries of time bins
//      (pml_sample_histories_through_time), launch_scenarios into d_states [N][rs] included (d_fallback: its counter, zeroed).  host: the caller's -- plan, ends and pieces (cut by history_time_sample_piece(N), with
//      the pseudo-bin if the lineages are asked for) filled in, the tables the launcher derives from them left to it --, alive until
//      the caller's scope has waited.  Device arrays d_times [n_rep][M][k], d_jumps [n_rep][M][k][k] (zeroed) or null, d_lineages
//      [n_rep][M + 1][k] (zeroed) or null, d_skipped: one counter (zeroed); queued only
struct HistoryTimeSamplePlan {
    PmlTimeSegments plan;
    PmlTimeSegmentEnds ends;
    PmlTimePieces pieces;
    std::vector<int> flags, piece_bin;
    std::vector<double> pos;
};
PML_INTERNAL int history_time_sample_piece(int N);
PML_INTERNAL int launch_history_time_sample(pml_ctx* ctx, CallScope& mem, int col, int n_rep, int rep_offset, u64 seed,
                                            void* d_states, size_t rs, HistoryTimeSamplePlan& host, double* d_times,
                                            unsigned* d_jumps, unsigned* d_lineages, unsigned long long* d_fallback,
                                            unsigned long long* d_skipped);

// More than 64 KB of dynamic LDS must be asked for: once per kernel, device and size (the largest asked for so far is what is
// set) -- not per launch: the call is not free and should not sit inside a stream capture.  (A template: one table per kernel
// type and translation unit; the kernels that share a type are told apart by their address.)
template <typename K>
static inline int with_lds(const pml_ctx* ctx, K kernel, size_t bytes) {
    struct Entry {
        const void* fn;
        int device;
        size_t bytes;
    };
    static std::mutex mu;
    static std::vector<Entry> done;
    std::lock_guard<std::mutex> lock(mu);
    Entry* e = nullptr;
    for (auto& d : done)
        if (d.fn == (const void*)kernel && d.device == ctx->device) e = &d;
    if (e != nullptr && e->bytes >= bytes) return PML_OK;
    HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (e != nullptr) e->bytes = bytes;
    else done.push_back(Entry{(const void*)kernel, ctx->device, bytes});
    return PML_OK;
}

// a level launch over the entries first .. first + n_level of a list: its unit descriptors (F81 family) or its node ids
static inline int dispatch_sweep(pml_ctx* ctx, SweepKind what, int list, int first, int n_level, bool cherries = true,
                                 bool bu_sweep = false, int window = -1) {
    if (n_level <= 0) return PML_OK;
    if (ctx->kind == PML_MODEL_F81) return dispatch_sweep_f81(ctx, what, ctx->d_unit_lists[list] + first, n_level, cherries, bu_sweep);
    const int* nodes = list == L_BU_PLAIN ? ctx->d_bu_order : (list == L_TD_PLAIN ? ctx->d_td_parents : nullptr);
    return dispatch_sweep_matrix(ctx, what, nodes ? nodes + first : nullptr, n_level, window);
}
