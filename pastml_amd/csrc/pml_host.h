// Host side shared by the translation units of libpastml_hip.so: the context behind the opaque pml_ctx, its switches, the
// small helpers every launcher needs.  gfx950 only.  (Round 6: the library was one 5 000-line translation unit that took
// 3.5 minutes to compile; the kernel families now sit in translation units of their own, pml_launch_*.hip, built in
// parallel by pastml_amd/build.py -- this header is what they share with pml_api.hip.)
#pragma once
#include "../../include/pastml_hip.h"

#include <algorithm>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <string>
#include <chrono>
#include <vector>

#include "pml_model.h"   // PmlTree, PmlCols, PmlState, PmlUnit, PmlModel (and the F81 / miscellaneous kernels' headers below it)
#include "pml_schedule.h" // PmlTune, the schedules' host side, PmlForest
#include "pml_columns.h"  // PmlColumnPlan: lane shapes, padding, the parameter block's layout
#include "pml_pij_window.h" // PmlWindowStep
#include "pml_results.h"   // PmlResults: what the result buffers hold

struct PmlComm;  // pml_comm.h (pml_api.hip only)

// How the stream is being captured while a sweep is enqueued: not at all (the sweep may replay a graph of its own), into the
// sweep's own graph, or into the one graph of a whole marginal pass (the sweeps inside it keep no graphs of their own).
enum PmlCapture { CAP_NONE, CAP_OWN, CAP_PASS };

#define PML_VERSION 104

// internal linkage across the library's translation units (not part of the C-ABI)
#define PML_INTERNAL __attribute__((visibility("hidden")))

// records the message pml_last_error() returns on this thread and hands `code` back (defined in pml_api.hip)
PML_INTERNAL int pml_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define fail pml_fail

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess)                                                                                 \
            return fail(PML_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define PML_TRY(expr)            \
    do {                         \
        int _s = (expr);         \
        if (_s != PML_OK) return _s; \
    } while (0)

struct pml_ctx {
    int device = 0;
    PmlTune tune;  // the schedules' switches (environment at creation, pml_ctx_set_tunable)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // kernel timing (pml_profile_*): event pairs around the level launches, read back when the profile is read -- a
    // bracket never makes the host wait inside a sweep
    struct ProfBracket {
        hipEvent_t a, b;
        int which;
        long long launches;
    };
    std::vector<ProfBracket> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    hipEvent_t prof_open = nullptr;
    bool profile = false;
    double prof_ms[5] = {0, 0, 0, 0, 0};  // bottom-up levels, top-down levels, per-branch pass, two-level launch TD / BU
    long long prof_launches[5] = {0, 0, 0, 0, 0};
    std::vector<void*> allocs;
    size_t held = 0;

    // tree
    int N = 0, n_roots = 0, n_bu_levels = 0, n_td_levels = 0;
    int *d_parent = nullptr, *d_first_child = nullptr, *d_n_children = nullptr, *d_post_rank = nullptr;
    int *d_bu_order = nullptr, *d_td_parents = nullptr;
    int* d_tips = nullptr;  // ids of the tips (the fused eigen sweeps give them a launch of their own)
    int *d_bu_offsets = nullptr, *d_td_offsets = nullptr;  // level tables on the device (narrow end in one launch)
    int n_tips = 0;
    double* d_msg = nullptr;  // fused eigen sweeps: messages of the bottom-up sweep
    int *d_tip_rest = nullptr, *d_tip_rest_count = nullptr;  // eigen joint sweep: [C][n_tips] tips that are not observed, [C]
    double* d_dist = nullptr;
    PmlForest forest;  // the forest in the library's numbering (pml_plan_forest): level tables, kinds, fused lists, traits
    // Internal node numbering (height_order below): the library numbers the nodes of a ragged forest so that the sibling
    // groups a level's units gather lie next to each other; every per-node array that crosses the C-ABI is in the CALLER's
    // numbering and is permuted on the way in / out.  Both empty when the caller's numbering is kept (balanced trees, ...).
    std::vector<int> new_of_old, old_of_new;
    int *d_new_of_old = nullptr, *d_old_of_new = nullptr;   // the same on the device (outputs are permuted there: gather_rows_kernel)
    void* d_stage = nullptr;   // one column's rows in the caller's numbering, on their way out
    size_t stage_bytes = 0;
    // cherry fusion (F81 marginal sweeps): node kinds and level lists over the stored internal nodes only
    bool fuse = true;
    unsigned char* d_kind = nullptr;
    int *d_bu_order_f = nullptr, *d_td_parents_f = nullptr, *d_cherries = nullptr;
    // unit descriptors of the F81 kernels, parallel to d_bu_order_f / d_td_parents_f / d_bu_order
    PmlUnit *d_bu_units_f = nullptr, *d_td_units_f = nullptr, *d_bu_units = nullptr, *d_cherry_units = nullptr;
    // the same fused lists with every level's units sorted by shape (level launches of wide units, see pml_tree_upload)
    PmlUnit *d_bu_units_fs = nullptr, *d_td_units_fs = nullptr;
    int *d_bu_offsets_f = nullptr, *d_td_parent_offsets_f = nullptr;  // level tables for the single-launch kernels
    // the schedules the sweeps walk (pml_schedule.h): planned by pml_schedule.cpp, uploaded by pml_tree_upload / build_thin_ends
    using BlockSchedule = PmlBlockSchedule;
    using ThinSchedule = PmlThinSchedule;
    using DeepSchedule = PmlDeepSchedule;
    using SuperSchedule = PmlSuperSchedule;
    using EigenTiers = PmlEigenTiers;
    using BacktraceTiers = PmlBacktraceTiers;
    BlockSchedule blocks;
    ThinSchedule thin;
    DeepSchedule deep;
    SuperSchedule sup;
    EigenTiers eig_tiers;
    BacktraceTiers bt_tiers;
    bool small = false;  // forest small enough for the one-launch-per-sweep kernels
    std::vector<char> bu_level_vec_f;  // per fused bottom-up level: some unit has a stored node as child 0 or 1
    std::vector<int> td_cherry_prefix; // over the fused top-down units: how many before it have a cherry as child 0 or 1
    std::vector<char> bu_level_vec;    // the same for the plain levels (joint sweep: every internal node is stored)
    int n_cherries = 0;

    // columns
    PmlColumnPlan cols;   // what pml_plan_columns decided (pml_chars_alloc): lane shapes, flags, the parameter block's layout
    int C = 0, k = 0, ks = 0, W = 0;   // copies of the plan's, read everywhere
    u64 *d_masks = nullptr, *d_masks_init = nullptr;
    bool has_init = false;
    int kind = -1;
    double *d_pi = nullptr, *d_mu = nullptr, *d_kappa = nullptr, *d_d = nullptr, *d_A = nullptr, *d_Ainv = nullptr;
    double* d_active = nullptr;   // last array of the parameter block: 0.0 = the column sits the next bottom-up sweep out
    bool active_partial = false;  // ... some column does (pml_bottom_up_submit_columns)
    int n_active = 0;             // columns that take part in the next sweep
    int sched_cols = 0;           // the number of columns the schedule of a sweep is chosen for (C; 32 for a few active ones)
    std::vector<double> h_eig_d;  // [C][k]: the eigenvalues pml_model_set_eigen was given (pml_expected_history_eigen checks them)
    double* d_Asym = nullptr;   // [C][k][k], 65 <= k <= 128: the one matrix of the sum sweeps (eig_sym_kernel)
    double* d_eigT = nullptr;   // [C][k][k]: scratch of that kernel
    std::vector<double> h_symA; // [C][k k + k]: the A and pi d_Asym was made from (an unchanged model is not orthonormalised again)
    std::vector<char> eig_sym;  // per column: the identity holds for the matrices pml_model_set_eigen was given
    bool eig_sym_all = false;   // ... for every column: the sum sweeps of 65 - 128 states keep one matrix in LDS
    double* d_AinvT = nullptr;  // [C][ld][ld], ld = 32 (k <= 32) or 64 (k <= 64): Ainv transposed and zero-padded -- eigen_joint_kernel (k <= 32), eigen_gemm_kernel's observed tips
    double* d_AT = nullptr;     // [C][32][32]: A transposed and zero-padded (k <= 32), for pij_eigen_valu_kernel
    double *d_sf = nullptr, *d_tau = nullptr, *d_tauf = nullptr;
    std::vector<char> model_set;  // per column
    std::vector<char> tips_observed;  // per column: every tip has exactly one allowed state (known from pml_masks_from_tip_states)
    // P(t) in a window instead of the batch (pml_pij_window.h; eigen models beyond 32 states, pml_pij_window_set): B branches per
    // column; the branch lists of the bottom-up [0] and the top-down [1] level lists in run order, and the per-node slot tables
    long long pij_window = 0;            // B; 0 = the batch of the whole tree (d_P)
    long long pij_window_tuned = -1;     // the value of PASTML_HIP_PIJ_WINDOW that was applied last (window_from_tunable)
    double* d_pij_window = nullptr;      // [C][B][k][ks]
    int *d_win_branches[2] = {nullptr, nullptr}, *d_win_slot[2] = {nullptr, nullptr};
    std::vector<int> win_branches[2];    // host copies: a sweep's windowed plan must list what was uploaded
    std::vector<int> bu_order, td_parents;   // the plain level lists on the host (library's numbering), for the window planner
    // the windowed sequences already cut for this window, by the plan they were cut from (a sweep's plan is a few records per
    // level; cutting it is O(N)): an uncaptured sweep plans its runs once, not per likelihood evaluation.  Dropped with the window.
    struct WindowCut {
        std::vector<PmlLaunch> plan;
        std::vector<PmlWindowStep> steps;
    };
    std::vector<WindowCut> win_cuts;
    // the runs of the plain top-down level list the slot table [1] was made for: pml_marginal_counts walks them (window_set)
    std::vector<PmlWindowStep> win_td_runs;

    // state
    double *d_E = nullptr, *d_P = nullptr, *d_bu = nullptr, *d_S = nullptr, *d_td = nullptr, *d_post = nullptr,
           *d_lhsum = nullptr;
    i64 *d_be = nullptr, *d_te = nullptr, *d_lhe = nullptr;
    pml_jt* d_J = nullptr;  // arg-max tables, one byte per entry (two beyond 256 states)
    int* d_js = nullptr;
    u64* d_err = nullptr;
    PmlResults results;  // which of these hold a valid sweep's results, and which rows the sweeps left out of memory
    int* d_nsel = nullptr;
    // hipGraph replay of the launch sequence of a sweep (level kernels are launch-bound on mid-size trees)
    struct GraphSlot {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        bool has_init = false;
        PmlSweepOutcome outcome;  // of the captured sequence (run_captured hands it out, captured just now or replayed)
    };
    GraphSlot bu_graph[2], td_graph, bt_graph;
    GraphSlot bu_graph_few;        // the marginal sweep as scheduled for a few active columns (submit_bottom_up)
    GraphSlot mp_graph;            // bottom-up + top-down of pml_marginal_pass as ONE graph
    bool graphs = true;
    double* h_loglik = nullptr;  // pinned staging of the per-column results
    // behind them, in the same allocation: the bad-tip word of the F81 top-down kernels (post_onehot).  The host clears it before
    // a top-down sweep goes on the stream and reads it behind the wait for that sweep (begin_top_down / end_top_down).
    u64* h_bad_tip = nullptr;
    // pi, sf, tau, tau factor, mu, kappa of all columns live in ONE device block with a pinned host mirror of the same
    // layout (cols.params, PmlParamBlock): a parameter update (every optimiser step) is one asynchronous copy and no
    // synchronisation.  Behind them the flags of the active columns and, last, one word for the top-down sweep: the observed
    // tips' rows are kept.
    double *d_params = nullptr, *h_params = nullptr;
    bool params_dirty = false;  // the pinned mirror holds values the device block has not seen (params_push sends them)
    u64* h_err = nullptr;
    // completion of a bottom-up sweep whose last launch is the single-workgroup-per-column kernel: that kernel raises a
    // word in pinned memory when its last column is done (bu_f81_small_kernel), and the collect spins on it
    u64* h_done = nullptr;      // pinned: generation of the last finished launch
    u64* d_done = nullptr;      // device: [0] columns done in the running launch, [1] generation
    // the same for a whole marginal pass: its last top-down launch signals where the schedule ends in a multi-level
    // kernel (single-launch sweeps, subtree blocks); the word counts the signalling launches (PmlSweepOutcome::n_signals)
    struct Pending {
        u64 expect = 0;     // what *h_done shows when what was submitted last has finished
        bool spin = false;  // its end raises the word and nobody has waited for it yet: wait_pending spins
    } pending;
    bool keep_td = false;      // PML_OPT_KEEP_TD (or a pml_download of the TD vectors asked for them)
    bool eig_fused_opt = true; // PML_OPT_EIGEN_FUSED
    bool eigj_valu_opt = true; // PML_OPT_EIGEN_JOINT_VALU
    bool implicit_tips = false;    // PML_OPT_IMPLICIT_TIP_POSTERIORS
    const PmlUnit* d_unit_lists[L_COUNT] = {};   // the unit lists of the F81 kernels by PmlList (pml_tree_upload)
    const int* d_list_offsets[L_COUNT] = {};     // ... and the level tables of those that several-level launches walk

    // forward simulation (pml_launch_simulate.hip): preorder node lists of the subtrees rooted at depth sim_depth (built on
    // first use for that depth; a new tree resets them)
    int sim_depth = -1, sim_n_lists = 0;
    int4* d_sim_lists = nullptr;   // (internal id, caller's id, caller's id of the parent, 0) per node
    int* d_sim_off = nullptr;

    // parsimony (pml_launch_parsimony.hip): kernel launches and event time of the passes of the last pml_parsimony
    long long pars_launches = 0;
    double pars_ms = 0;
    // vertical collapse (pml_launch_compress.hip): event times of the merged pass, the pointer jumping and the counts of the
    // last pml_compress_vertical (zero unless the context profiles), and its number of jumping rounds
    double compress_ms[3] = {0, 0, 0};
    int compress_rounds = 0;
    // horizontal merging (pml_launch_compress_horizontal.hip), last pml_compress_horizontal: event times of the labelling of the
    // states, the level loop and the pass down (zero unless the context profiles), levels, kernel launches, slots of the table
    double hz_ms[3] = {0, 0, 0};
    int hz_levels = 0;
    long long hz_launches = 0, hz_slots = 0;
    // trimming (pml_launch_compress_trim.hip), last pml_compress_trim: event times of the sizes, the removal and the mediators
    // (zero unless the context profiles), levels of the vertex forest, rounds of the multiplier, kernel launches
    double trim_ms[3] = {0, 0, 0};
    int trim_levels = 0, trim_rounds = 0;
    long long trim_launches = 0;
    // timeline (pml_launch_timeline.hip), last pml_timeline: event times of the dates, get_date, the bins, the role counts, the
    // tips below and the vertices (zero unless the context profiles), levels, kernel launches, those of the date sweep
    double tl_ms[6] = {0, 0, 0, 0, 0, 0};
    int tl_levels = 0;
    long long tl_launches = 0, tl_date_launches = 0;

    PmlComm* comm = nullptr;   // RCCL communicator attached by pml_comm_init (survives tree uploads)
};

#include "pml_call_scope.h"   // the scratch and events of ONE call (what the context itself holds: dev_alloc below)

// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
static int dev_alloc(pml_ctx* ctx, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T));
    if (e != hipSuccess)
        return fail(PML_ERR_HIP, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
    ctx->allocs.push_back(q);
    ctx->held += count * sizeof(T);
    *p = (T*)q;
    return PML_OK;
}

// gives back one of the context's own allocations before the context goes
template <typename T>
static void dev_release(pml_ctx* ctx, T** p, size_t count) {
    if (!*p) return;
    for (size_t i = 0; i < ctx->allocs.size(); ++i)
        if (ctx->allocs[i] == (void*)*p) {
            ctx->allocs.erase(ctx->allocs.begin() + (long)i);
            break;
        }
    (void)hipFree((void*)*p);
    const size_t bytes = (count ? count : 1) * sizeof(T);
    ctx->held -= std::min(ctx->held, bytes);
    *p = nullptr;
}

static void drop_graph(pml_ctx::GraphSlot& g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
    g.exec = nullptr;
    g.graph = nullptr;
}

// every captured launch sequence of the two sweeps (the back-trace's graph depends on the tree and the tunables only)
static void drop_sweep_graphs(pml_ctx* ctx) {
    drop_graph(ctx->bu_graph[0]);
    drop_graph(ctx->bu_graph[1]);
    drop_graph(ctx->bu_graph_few);
    drop_graph(ctx->td_graph);
    drop_graph(ctx->mp_graph);
}

static int prof_drain(pml_ctx* ctx);

static void free_all(pml_ctx* ctx) {
    drop_sweep_graphs(ctx);
    drop_graph(ctx->bt_graph);
    if (ctx->h_loglik) (void)hipHostFree(ctx->h_loglik);
    if (ctx->h_err) (void)hipHostFree(ctx->h_err);
    if (ctx->h_done) (void)hipHostFree(ctx->h_done);
    ctx->h_done = nullptr;
    if (ctx->h_params) (void)hipHostFree(ctx->h_params);
    ctx->h_params = nullptr;
    ctx->h_loglik = nullptr;
    ctx->h_bad_tip = nullptr;
    ctx->h_err = nullptr;
    for (void* p : ctx->allocs) (void)hipFree(p);
    if (ctx->d_stage) (void)hipFree(ctx->d_stage);
    ctx->d_stage = nullptr;
    ctx->stage_bytes = 0;
    if (ctx->d_sim_lists) (void)hipFree(ctx->d_sim_lists);
    if (ctx->d_sim_off) (void)hipFree(ctx->d_sim_off);
    ctx->d_sim_lists = nullptr;
    ctx->d_sim_off = nullptr;
    ctx->sim_depth = -1;
    ctx->allocs.clear();
    ctx->held = 0;
}

// A new tree: everything the ctx holds goes, except what belongs to the context rather than to a tree -- the device, the
// settings (tunables, options, profiling), the stream and its events, the profiling event pool and the communicator.
static void reset_for_tree(pml_ctx* ctx) {
    free_all(ctx);
    (void)prof_drain(ctx);
    pml_ctx fresh;
    fresh.device = ctx->device;
    fresh.tune = ctx->tune;
    fresh.fuse = ctx->fuse;
    fresh.keep_td = ctx->keep_td;
    fresh.eig_fused_opt = ctx->eig_fused_opt;
    fresh.eigj_valu_opt = ctx->eigj_valu_opt;
    fresh.implicit_tips = ctx->implicit_tips;
    fresh.profile = ctx->profile;
    fresh.stream = ctx->stream;
    fresh.ev0 = ctx->ev0;
    fresh.ev1 = ctx->ev1;
    fresh.prof_pool.swap(ctx->prof_pool);
    if (ctx->prof_open) fresh.prof_pool.push_back(ctx->prof_open);
    fresh.comm = ctx->comm;
    *ctx = std::move(fresh);
}

template <typename T>
static int upload(pml_ctx* ctx, T* dst, const T* src, size_t count) {
    HIP_TRY(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return PML_OK;
}

// a table of a tree on the device: allocated (at least one element) and its copy queued; the caller synchronises the
// stream before the host table goes
template <typename T>
static int put(pml_ctx* ctx, T** dst, const T* src, size_t count) {
    PML_TRY(dev_alloc(ctx, dst, count));
    if (count) PML_TRY(upload(ctx, *dst, src, count));
    return PML_OK;
}
template <typename T>
static int put(pml_ctx* ctx, T** dst, const std::vector<T>& v) {
    return put(ctx, dst, v.data(), v.size());
}

// Blocks along x for a level of n_units units per column (grid-stride loops take the rest).  The cap on the total
// number of blocks was measured on cfg4 (MI355X): the pipelined kernels (bottom-up, and the top-down two-level kernel)
// like ~8192 (a wave then walks several units and its prefetch stage pays off), everything else 32768; persistent-size
// grids (768-2048) were 5-15 % slower.
static int grid_for(const pml_ctx* ctx, int n_units, int units_per_block, int C, bool pipelined = false) {
    int blocks = (n_units + units_per_block - 1) / units_per_block;
    const int cap_env = (int)ctx->tune.get(T_GRID_CAP, 0);
    const int total_cap = cap_env > 0 ? cap_env : (pipelined ? 8192 : 32768);
    int cap = total_cap / (C < 1 ? 1 : C);
    if (cap < 8) cap = 8;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return blocks;
}

// Whole F81 sweeps in ONE launch (one workgroup per column walks every level): forests of up to
// PASTML_HIP_SMALL_MAX_NODES (2048) nodes, where a sweep is otherwise a chain of latency-bound launches -- and, when
// there are many columns (the optimiser's batches: one workgroup per column already fills the chip), forests of up to
// PASTML_HIP_SMALL_MANY_NODES (16384) nodes whose levels each fit one pass of a workgroup (deep, ragged trees:
// HIV1C-sized sweeps -- 7 237 nodes, 57 height levels -- of 246 binary columns 0.34 -> 0.27 ms; a balanced 4 096-tip
// tree with 20 states has levels of 16 passes and stays with the level kernels: 0.12 against 0.27 ms).  Same unit
// functions and lane shapes as the level kernels: identical bits.
// (more than 256 states -- round 6, the F81 family only, 64 lanes x 8 states -- run the plain level schedule: their one lane
// shape is instantiated for the level kernels alone)
static inline bool wide_states(const pml_ctx* c) { return c->k > 256; }

static bool single_launch_sweeps(const pml_ctx* c) {
    if (wide_states(c)) return false;
    const int many = (int)c->tune.get(T_SMALL_MANY_NODES, 16384);
    return c->small || (c->sched_cols >= 64 && c->N <= many && c->cols.levels_fit_workgroup);
}

// The subtree-block schedule pays where a sweep is a chain of latency-bound launches; once the levels carry enough work
// to fill the chip (stored nodes x columns beyond ~1.6e5: measured on 16 384 - 131 072-tip trees with 1 - 32 columns)
// the level kernels, which spread every level over all compute units, win again.
static bool block_schedule(const pml_ctx* c) {
    const long long limit = c->tune.get(T_BLOCK_MAX_WORK, 160000);
    // (Round 2 also capped the number of (block, level, column) workgroup steps: with 512-thread workgroups a ragged tree
    // times many columns ran in rounds of long-lived workgroups and lost to the level kernels.  The workgroups now
    // shrink until all are resident (launch_blocks_f81) and the blocks end below the top's lowest level
    // (pml_tree_upload): over scripts/schedule_sweep.py's grid the blocks never lose -- profiles/r03c_schedule_sweep.txt.)
    return c->blocks.ok && !wide_states(c) && !c->forest.bu_offsets_f.empty() && (long long)c->forest.bu_offsets_f.back() * c->sched_cols <= limit;
}

static PmlTree tree_of(const pml_ctx* c, bool fused = false) {
    PmlTree t;
    t.kind = fused ? c->d_kind : nullptr;
    t.N = c->N;
    t.n_roots = c->n_roots;
    t.parent = c->d_parent;
    t.first_child = c->d_first_child;
    t.n_children = c->d_n_children;
    t.dist = c->d_dist;
    t.post_rank = c->d_post_rank;
    return t;
}

// bu_sweep: the launch is part of a bottom-up sweep, which looks at the flags of the active columns
static PmlCols cols_of(const pml_ctx* c, bool bu_sweep = false) {
    PmlCols s;
    s.k = c->k;
    s.ks = c->ks;
    s.W = c->W;
    s.no_wide_lean = c->tune.on(T_NO_WIDE_LEAN) ? 1 : 0;
    s.masks = c->d_masks;
    s.masks_init = c->has_init ? c->d_masks_init : nullptr;
    s.pi = c->d_pi;
    s.active = bu_sweep ? c->d_active : nullptr;  // (only the sweep itself: downloads rebuild what they need for all)
    return s;
}

static PmlState state_of(const pml_ctx* c) {
    PmlState s;
    s.E = c->d_E;
    s.bu = c->d_bu;
    s.S = c->d_S;
    s.be = c->d_be;
    // F81 family: the top-down sweep runs on the stored posteriors; TD vectors are written only on request
    const bool td_stored = c->kind != PML_MODEL_F81 || c->keep_td;
    s.td = td_stored ? c->d_td : nullptr;
    s.te = td_stored ? c->d_te : nullptr;
    s.post = c->d_post;
    s.implicit_tips = c->implicit_tips && c->kind == PML_MODEL_F81 && c->W == 1;
    s.keep_tips = PmlParamBlock::at(c->d_params, c->cols.params.keep_tips);   // last word of the block (begin_top_down sets it)
    s.bad_tip = c->h_bad_tip;
    s.lhsum = c->d_lhsum;
    s.lhe = c->d_lhe;
    s.J = c->d_J;
    s.jt16 = c->k > 256;
    s.js = c->d_js;
    s.err = c->d_err;
    s.msg = c->d_msg;
    return s;
}

// Eigen models with 16 <= k <= 32 run the fused matrix-core sweeps (pml_kernels_eigen_mfma.h): P(t) is built and
// consumed in registers.  PASTML_HIP_NO_MFMA / PASTML_HIP_NO_EIGEN_FUSED fall back to the materialised-P kernels.
static bool eigen_fused(const pml_ctx* c) {
    const bool off = c->tune.on(T_NO_MFMA) || c->tune.on(T_NO_EIGEN_FUSED);
    return !off && c->eig_fused_opt && c->kind == PML_MODEL_EIGEN && c->k >= 16 && c->k <= 32 && c->W == 1 &&
           c->ks == 4 * ((c->k + 3) / 4);
}

// HKY sweeps build P(t) in registers (pml_kernels_matrix.h, PML_P_HKY); PASTML_HIP_NO_HKY_FUSED reads the batch.
static bool hky_fused(const pml_ctx* c) {
    const bool off = c->tune.on(T_NO_HKY_FUSED);
    return !off && c->kind == PML_MODEL_HKY && c->k == 4 && c->ks == 4 && c->cols.G == 4 && c->cols.R == 1 && c->W == 1;
}

static PmlModel model_of(const pml_ctx* c) {
    PmlModel m;
    m.kind = c->kind;
    m.mu = c->d_mu;
    m.kappa = c->d_kappa;
    m.d = c->d_d;
    m.A = c->d_A;
    m.Ainv = c->d_Ainv;
    m.AinvT = c->d_AinvT;
    m.Asym = c->d_Asym;
    m.ldT = c->k <= PML_EIGJ_STRIDE ? PML_EIGJ_STRIDE : 64;
    m.sf = c->d_sf;
    m.tau = c->d_tau;
    m.tauf = c->d_tauf;
    return m;
}

static int prof_event(pml_ctx* ctx, hipEvent_t* out) {
    if (!ctx->prof_pool.empty()) {
        *out = ctx->prof_pool.back();
        ctx->prof_pool.pop_back();
        return PML_OK;
    }
    HIP_TRY(hipEventCreate(out));
    return PML_OK;
}

// adds up the brackets recorded so far (waits for the stream) and returns their events to the pool
static int prof_drain(pml_ctx* ctx) {
    if (ctx->prof_pending.empty()) return PML_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    for (const pml_ctx::ProfBracket& br : ctx->prof_pending) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(br.b));
        HIP_TRY(hipEventElapsedTime(&ms, br.a, br.b));
        ctx->prof_ms[br.which] += ms;
        ctx->prof_launches[br.which] += br.launches;
        ctx->prof_pool.push_back(br.a);
        ctx->prof_pool.push_back(br.b);
    }
    ctx->prof_pending.clear();
    return PML_OK;
}

static void prof_release(pml_ctx* ctx) {
    for (const pml_ctx::ProfBracket& br : ctx->prof_pending) {
        (void)hipEventDestroy(br.a);
        (void)hipEventDestroy(br.b);
    }
    for (hipEvent_t e : ctx->prof_pool) (void)hipEventDestroy(e);
    if (ctx->prof_open) (void)hipEventDestroy(ctx->prof_open);
    ctx->prof_pending.clear();
    ctx->prof_pool.clear();
    ctx->prof_open = nullptr;
}

static int prof_begin(pml_ctx* ctx) {
    if (!ctx->profile) return PML_OK;
    if (!ctx->prof_open) PML_TRY(prof_event(ctx, &ctx->prof_open));
    HIP_TRY(hipEventRecord(ctx->prof_open, ctx->stream));
    return PML_OK;
}

static int prof_end(pml_ctx* ctx, int which, long long launches) {
    if (!ctx->profile || !ctx->prof_open) return PML_OK;
    hipEvent_t b = nullptr;
    PML_TRY(prof_event(ctx, &b));
    HIP_TRY(hipEventRecord(b, ctx->stream));
    ctx->prof_pending.push_back({ctx->prof_open, b, which, launches});
    ctx->prof_open = nullptr;
    if (ctx->prof_pending.size() >= 4096) PML_TRY(prof_drain(ctx));  // (bounds the number of live events)
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// What pml_api.hip defines and the entries that read a marginal pass (pml_api_readers.hip) call as well; each is described where
// it is defined.
PML_INTERNAL int require_model(pml_ctx* ctx);
PML_INTERNAL int check_cols(pml_ctx* ctx, int cb, int ce);
PML_INTERNAL int wait_pending(pml_ctx* ctx, bool idle = false);
PML_INTERNAL int window_from_tunable(pml_ctx* ctx);
PML_INTERNAL int consumer_prep(pml_ctx* ctx, bool force = false);
PML_INTERNAL int materialize_cherries(pml_ctx* ctx);
PML_INTERNAL int materialize_tip_posteriors(pml_ctx* ctx);
template <typename T>
PML_INTERNAL int fetch_rows(pml_ctx* ctx, const T* d_src, size_t src_width, size_t width, size_t n_cols, T* out);   // (T: double, i64, int)
