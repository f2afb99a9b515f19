// Tree schedules, planned on the host: the library's numbering of a forest, its fused level lists, the unit descriptors and
// every schedule the sweeps walk (eigen joint tiers, back-trace tiers, two-level and stacked units, subtree blocks, thin
// ends).  Plain C++ over plain tables: pml_tree_upload (pml_api.hip) calls the tree's planners and uploads what they return;
// pml_chars_alloc calls pml_plan_columns (pml_columns.h) and, where that plan asks for thin ends, pml_plan_thin_ends; the
// sweeps call the launch planners.  No HIP here, so that the planning can be built, tested and sanitised on any host.
#pragma once
#include <cstdlib>
#include <string>
#include <vector>

#define PML_KIND_TIP 0
#define PML_KIND_CHERRY 1
#define PML_KIND_STORED 2

// Unit descriptor, built once per tree on the host (pml_tree_upload): everything about the topology around node n that
// a unit needs, so that all data loads of a unit can be issued in one round trip (and the descriptor of the wave's next
// unit is fetched while the current one is computed) instead of chasing n -> first_child -> children -> their children.
//   packed: bits 0-3 number of children (15 = 15 or more), bit 4 = every cherry among the first four children has
//           1..GC tips, bit 5 = no stored internal node among children 2 and 3 (the bottom-up pipeline prefetches the
//           vectors of children 0 and 1), bits 8+3j..10+3j (j < 4) code of child j: 0 tip, 1 stored internal node,
//           2+m cherry with m+1 tips
//   cfc[j]: first child of child j (j < 4), i.e. where the tips of a cherry child start
struct __attribute__((aligned(32))) PmlUnit {
    int n, fc, packed, pad;
    int cfc[4];
};

#define PML_PACKED_TWO_STORED ((1 << 11) | (1 << 8) | (3 << 4) | 2)  // two children, both stored nodes

// threads of the workgroup that walks several levels in one launch (pml_kernels_f81.h: the single-launch kernels and the
// subtree blocks); here because pml_plan_columns counts a level's passes of it
#define PML_SMALL_BLOCK 512

// ---------------------------------------------------------------------------------------------------------------------
// Every switch of the schedules in one table per context.  The defaults come from the environment (PASTML_HIP_<NAME>) when
// the ctx is created, the C-ABI's set_tunable overrides them for that ctx -- there are no function-local statics: two contexts
// of one process can run different schedules, and a test that sets a switch gets it (round 3 latched several of them at
// their first use in the process).  FLAG: on when present (environment: whatever the value; set_tunable: value != 0).
// TREE: read by pml_tree_upload / pml_chars_alloc, so it must be set before the tree is uploaded.
// ---------------------------------------------------------------------------------------------------------------------
#define PML_TUNABLES(X)                                                                                              \
    X(GRID_CAP, 0, 0) X(SMALL_MANY_NODES, 0, 0) X(BLOCK_MAX_WORK, 0, 0)    \
    X(NO_MFMA, 1, 0) X(NO_EIGEN_FUSED, 1, 0) X(NO_HKY_FUSED, 1, 0)      \
    X(BLOCK_THREADS, 0, 0) X(EIG_BLOCKS, 0, 0) X(NO_EIGEN_GEMM, 1, 0) X(NO_EIGEN_JOINT_VALU, 1, 0) X(EIGJ_BLOCKS, 0, 0) \
    X(EIGJ_TIP_BLOCKS, 0, 0) X(EIGJ_ONE_TIPS_KERNEL, 1, 0) X(EIGJ_TIER_THIN, 0, 1) X(EIGJ_TIER_DEPTH, 0, 1)            \
    X(NO_EIGJ_TIERS, 1, 1) X(NO_BT_TIERS, 1, 1) X(NO_SHAPE_SORT, 1, 1) X(NO_SUPER, 1, 1) X(SUPER_MIN, 0, 1)            \
    X(STACK_MIN, 0, 1) X(NO_STACK, 1, 1) X(DEBUG, 1, 0) X(BLOCK_NODES, 0, 1) X(BLOCK_MAX_STORED, 0, 1)                 \
    X(BLOCK_HEIGHT_CAP, 0, 1) X(SMALL_MAX_NODES, 0, 1) X(F81_R, 0, 1) X(F81_TD_R, 0, 1) X(NO_GRAPH, 1, 1)              \
    X(NARROW_UNITS, 0, 0) X(NO_EIGG_TIERS, 1, 0) X(NO_SPIN_WAIT, 1, 0)   \
    X(PIJ_STAGE_ROWS, 0, 0) X(PIJ_BLOCKS, 0, 0) X(NO_HEIGHT_ORDER, 1, 1) X(NO_TD_TAIL, 1, 0) X(NO_PIJ_VALU, 1, 0) X(PIJ_VALU, 1, 0) X(NO_PIJ_WIDE, 1, 0) X(NO_EIGJ_PIPE, 1, 0) \
    X(THIN_UNITS, 0, 1) X(THIN_BYTES, 0, 1) X(THIN_BLOCK_NODES, 0, 1) X(NO_THIN, 1, 0) X(NO_THIN_WIDE, 1, 0) X(BU_WIDE, 0, 1) X(SORT_LEVELS, 0, 1) X(NO_WIDE_LEAN, 1, 0) X(SHAPE_ORDER, 0, 1) \
    X(PARS_MAX_COLS, 0, 0) X(PARS_THIN, 0, 0) X(COMPRESS_MAX_COLS, 0, 0) X(COMPRESS_PLAIN_ATOMICS, 1, 0) \
    X(PIJ_WINDOW, 0, 0) X(NO_KEEP_TIP_ROWS, 1, 0) X(NO_TIP_LANES, 1, 0) X(NO_TD_SUPER_PIPE, 1, 0) X(NO_TD_CHAIN, 1, 0) X(NO_BU_CHAIN, 1, 0)
enum PmlTunable {
#define X(name, flag, tree) T_##name,
    PML_TUNABLES(X)
#undef X
    T_COUNT
};
static const char* const kTunableName[T_COUNT] = {
#define X(name, flag, tree) #name,
    PML_TUNABLES(X)
#undef X
};
static const bool kTunableFlag[T_COUNT] = {
#define X(name, flag, tree) flag != 0,
    PML_TUNABLES(X)
#undef X
};
static const bool kTunableTree[T_COUNT] = {
#define X(name, flag, tree) tree != 0,
    PML_TUNABLES(X)
#undef X
};
struct PmlTune {
    long long val[T_COUNT];
    bool has[T_COUNT];
    PmlTune() {
        for (int i = 0; i < T_COUNT; ++i) {
            const std::string var = std::string("PASTML_HIP_") + kTunableName[i];
            const char* e = getenv(var.c_str());
            has[i] = e != nullptr;
            val[i] = e ? atoll(e) : 0;
        }
    }
    bool on(int i) const { return has[i]; }
    long long get(int i, long long dflt) const { return has[i] ? val[i] : dflt; }
};

// ---------------------------------------------------------------------------------------------------------------------
// The schedules as the launchers read them (the context's BlockSchedule, ...): launch geometry on the host, the tables on the
// device.  The planners fill the geometry and leave the device pointers null; pml_tree_upload sets them.
// ---------------------------------------------------------------------------------------------------------------------
// subtree blocks (pml_kernels_f81.h, bottom): the stored nodes cut into subtrees of at most PML_BLOCK_NODES stored
// nodes, walked by one workgroup each, and the "top" above the cuts with level tables of its own
struct PmlBlockSchedule {
    bool ok = false;
    int n_blocks = 0;
    long long steps = 0;  // sum over the blocks of their levels: workgroup steps of one column's sweep
    PmlUnit *d_bu_units = nullptr, *d_td_units = nullptr;          // units of the blocks, block by block
    int *d_bu_start = nullptr, *d_bu_levels = nullptr, *d_bu_lv = nullptr;
    int *d_td_start = nullptr, *d_td_levels = nullptr, *d_td_lv = nullptr;
    PmlUnit *d_top_bu_units = nullptr, *d_top_td_units = nullptr;  // units of the top part, level by level
    int *d_top_bu_offsets = nullptr, *d_top_td_offsets = nullptr;
    std::vector<int> top_bu_offsets, top_td_offsets;               // host copies (launch geometry)
    std::vector<char> top_bu_vec;                                   // per top level: stored node among children 0, 1
};
// Thin ends of a large ragged forest, units of fewer than 8 lanes (round 5).  Bottom-up: the fused levels from
// floor_level on (each of at most PASTML_HIP_THIN_UNITS units) in tiers of subtree blocks, like `blocks` but of that
// part of the forest only and with several small subtrees per workgroup; the wide levels below stay level launches.
struct PmlThinSchedule {
    bool ok = false;
    int floor_level = 0;  // the fused levels below stay level launches
    int top_level = 0;    // ... and from this one on they are the narrow end's (level launches where still wide)
    struct Tier { int first_block, n_blocks; };
    std::vector<Tier> tiers;   // runs of levels, each cut into subtrees of at most THIN_BLOCK_NODES units: a launch per tier
    PmlUnit* d_units = nullptr;
    int *d_start = nullptr, *d_levels = nullptr, *d_lv = nullptr;
};
// Top-down: the depths from first_depth on (each of at most THIN_UNITS parents): the subtrees hanging at first_depth,
// packed into bins of about THIN_BLOCK_NODES units, ONE launch walks them all, a workgroup per (bin, column).
struct PmlDeepSchedule {
    bool ok = false;
    int first_depth = 0, n_blocks = 0;
    PmlUnit* d_units = nullptr;
    int *d_start = nullptr, *d_levels = nullptr, *d_lv = nullptr;
};
// two-level units (pml_kernels_f81.h): nodes with two stored children that each carry two cherries of two tips run
// both levels in one unit; they and their children leave the level lists ("rest" lists, same level structure)
struct PmlSuperSchedule {
    bool ok = false;
    int n = 0;
    PmlUnit* d_units = nullptr;
    PmlUnit* d_child_units = nullptr;  // the 2 n children of the two-level units, as units of their own (downloads)
    PmlUnit *d_bu_units_r = nullptr, *d_td_units_r = nullptr;
    PmlUnit *d_bu_units_rs = nullptr, *d_td_units_rs = nullptr;  // ... sorted by shape inside every level
    // stacked units (pml_kernels_f81.h): nodes with two plain stored children of two stored children each, by
    // bottom-up level and by depth; their children as units of their own for downloads
    int n_child_units = 0;  // entries of d_child_units: the children of the two-level units
    int n_stack = 0;
    PmlUnit *d_stack_bu = nullptr, *d_stack_td = nullptr, *d_stack_children = nullptr;
    std::vector<int> stack_bu_offsets, stack_td_offsets;
    // Chained top-down launch (td_f81_chain_kernel): the depth whose stacked units hand their grandchildren's rows to the
    // two-level units through LDS, or -1.  It is the deepest depth with stacked units, and only when entry m of its range
    // has exactly the two-level nodes of entries 4 m .. 4 m + 3 of d_units as grandchildren, in that order, and the range
    // covers all n of them (a balanced forest); a ragged forest keeps the two launches.
    int chain_depth = -1;
    // Chained bottom-up launch (bu_f81_chain_kernel): the fused level (index into stack_bu_offsets) whose stacked units take their
    // grandchildren's vectors from the two-level units through LDS, or -1.  It is the lowest level with stacked units, and only
    // when entry m of its range has exactly the two-level nodes of entries 4 m .. 4 m + 3 of d_units as grandchildren, in that
    // order, the range covers all n of them and its nodes are of one depth.  (Not chain_depth: the bottom-up lists are ordered by fused height, the top-down
    // lists by depth, and the two agree on balanced forests only.)
    int bu_chain_level = -1;
    int *d_bu_offsets_r = nullptr, *d_td_offsets_r = nullptr;
    std::vector<int> bu_offsets_r, td_offsets_r;
    std::vector<char> bu_level_vec_r;
};
// Joint sweep of the eigen models: the thin levels of a large forest (runs of levels of at most 4 096 nodes) in tiers
// of four levels; a tier is cut into subtree blocks and ONE launch walks them, a workgroup per (block, column) with a
// workgroup barrier between its levels -- a level costs a ~3.5 us pass instead of a ~7.5 us dependent launch.
struct PmlEigenTiers {
    bool ok = false;
    int first_level = 0;   // plain bottom-up level the first tier starts at
    int top_level = 0;     // ... and the level from which the single-workgroup launch takes over
    struct Tier { int first_block, n_blocks, depth; };
    std::vector<Tier> tiers;
    PmlUnit* d_units = nullptr;
    int *d_lv = nullptr, *d_start = nullptr;
    int* d_nodes = nullptr;  // the node ids parallel to d_units (the sum sweeps walk node lists)
    int widest = 0;        // nodes of the widest level inside the tiers
};
// joint back-trace: the depths beyond its single-workgroup launch in tiers of subtrees (joint_backtrace_blocks_kernel)
struct PmlBacktraceTiers {
    bool ok = false;
    int first_depth = 0;  // depths 1 .. first_depth - 1 stay with the single-workgroup launch
    struct Tier { int first_block, n_blocks, depth; };
    std::vector<Tier> tiers;
    int *d_nodes = nullptr, *d_lv = nullptr, *d_start = nullptr;
};

// ---------------------------------------------------------------------------------------------------------------------
// The tree arrays of the C-ABI (include/pastml_hip.h, pml_tree_upload), in the caller's numbering or, after
// pml_plan_forest, in the library's.
struct PmlTreeArrays {
    int n_nodes, n_roots, n_bu_levels, n_td_levels;
    const int *parent, *first_child, *n_children, *bu_offsets, *bu_order, *td_offsets, *td_parent_offsets, *td_parents,
        *post_rank;
    const double* dist;
};

// The library's numbering (height_order): the permutation (both empty when the caller's numbering is kept) and the
// renumbered arrays the PmlTreeArrays point at.
struct PmlNumbering {
    std::vector<int> old_of_new, new_of_old;
    std::vector<int> parent, first_child, n_children, bu_order, td_parents, post_rank;
    std::vector<double> dist;
};

// The forest in the library's numbering, what the schedules are planned from.  pml_tree_upload keeps it on the context:
// pml_chars_alloc, the thin ends and the forward simulation read it.
struct PmlForest {
    bool fuse = true;                    // cherry fusion (PML_OPT_CHERRY_FUSION)
    int N = 0, n_roots = 0, n_internal = 0;
    std::vector<int> parent, first_child, n_children;
    std::vector<int> bu_offsets, td_offsets, td_parent_offsets;   // the caller's level tables (heights, depths)
    std::vector<unsigned char> kind;     // PML_KIND_* per node
    std::vector<int> fh;                 // fused height of a stored node (1: only tips and cherries below), else 0
    std::vector<int> order_f;            // the stored nodes by fused height, ids ascending inside a height
    std::vector<int> bu_offsets_f;       // ... level l (height l + 1) of it
    std::vector<int> tdp;                // the stored nodes by depth (the top-down fused lists)
    std::vector<int> td_parent_offsets_f;
    bool shape_ordered = false;   // the numbering orders a depth's sibling groups by (shape, class) of the gathering unit
    bool polytomies = false;      // 15 % of the nodes with grandchildren have three or four children
    bool balanced_parts = false;  // a 32nd of the internal nodes are roots of the two-level pattern (two_level_root)
    int max_h() const { return (int)bu_offsets_f.size() - 1; }
    int n_stored() const { return bu_offsets_f.empty() ? 0 : bu_offsets_f.back(); }
};

// Groups of nodes (subtree blocks, bins), each walked as consecutive levels: list = the nodes group by group and level by
// level, start = per group its first entry in lv, lv = per group the list offset of every level and the end, levels =
// per group its number of levels.
struct PmlLevelTable {
    std::vector<int> list, start, levels, lv;
    template <class F>  // mem in ascending level(n); a level wherever it changes
    void add_runs(const int* mem, size_t count, F level) {
        start.push_back((int)lv.size());
        int nl = 0;
        for (size_t q = 0; q < count; ++q) {
            if (q == 0 || level(mem[q]) != level(mem[q - 1])) {
                lv.push_back((int)list.size());
                ++nl;
            }
            list.push_back(mem[q]);
        }
        lv.push_back((int)list.size());
        levels.push_back(nl);
    }
    template <class F>  // mem in ascending level(n); exactly the levels first .. first + n - 1, empty ones included
    void add_cells(const int* mem, size_t count, F level, int first, int n) {
        start.push_back((int)lv.size());
        size_t q = 0;
        for (int d = 0; d < n; ++d) {
            lv.push_back((int)list.size());
            for (; q < count && level(mem[q]) == first + d; ++q) list.push_back(mem[q]);
        }
        lv.push_back((int)list.size());
        levels.push_back(n);
    }
};

// Everything pml_tree_upload puts on the device besides the forest's own arrays, and the geometry that goes with it.
struct PmlTreePlan {
    std::vector<int> tips, cherries;
    // unit descriptors of the lists the F81 kernels walk: fused bottom-up / top-down, plain bottom-up, the cherries
    std::vector<PmlUnit> bu_units_f, td_units_f, bu_units, cherry_units;
    bool shape_sort = false;                    // the fused lists sorted by shape inside every level (level launches of wide units)
    std::vector<PmlUnit> bu_units_fs, td_units_fs;
    std::vector<char> bu_level_vec_f, bu_level_vec;   // per level: some unit has a stored node as child 0 or 1
    std::vector<int> td_cherry_prefix;          // over the fused top-down units: how many before it have a cherry as child 0 or 1
    bool small = false;                         // forest small enough for the one-launch-per-sweep kernels
    struct { PmlEigenTiers s; PmlLevelTable t; std::vector<PmlUnit> units; } eig;
    struct { PmlBacktraceTiers s; PmlLevelTable t; } bt;
    struct {
        PmlSuperSchedule s;
        bool lists = false;   // two-level or stacked units: the rest lists are uploaded
        std::vector<PmlUnit> units, child_units, bu_units_r, td_units_r, bu_units_rs, td_units_rs, stack_bu, stack_td,
            stack_children;
    } sup;
    struct { PmlBlockSchedule s; PmlLevelTable bu, td; std::vector<PmlUnit> bu_units, td_units, top_bu_units, top_td_units; } blocks;
};

// The thin ends of a large forest (pml_chars_alloc: they depend on the columns' bytes)
struct PmlThinPlan {
    PmlThinSchedule thin;
    PmlDeepSchedule deep;
    PmlLevelTable bu, td;
    std::vector<PmlUnit> bu_units, td_units;
};

// ---------------------------------------------------------------------------------------------------------------------
// A sweep's launch sequence as data: pml_plan_bottom_up / _top_down / _backtrace decide which launches a sweep consists of
// and in what order, run_plan (pml_api.hip) issues them.  PASTML_HIP_DEBUG prints a plan, one line per record.
// ---------------------------------------------------------------------------------------------------------------------
enum SweepKind {
    SW_BU_MARG, SW_BU_JOINT, SW_TD, SW_ROOTS, SW_BU_MARG_FUSED, SW_TD_FUSED, SW_BU_CHERRIES,
    SW_BU_MARG_FUSED_NOVEC,  // a fused level none of whose units has a stored node among its first two children
    SW_BU_JOINT_NOVEC,       // the same for a level of the joint sweep (the level whose children are all tips)
    SW_BU_JOINT_FUSED, SW_BU_JOINT_FUSED_NOVEC,  // joint sweep over the cherry-fused level lists
    SW_BU_CHERRIES_JOINT     // materialises the cherries' vectors after a fused joint sweep
};
enum PmlEigenFamily { EIG_JOINT, EIG_GEMM, EIG_FUSED };   // which eigen kernels an OP_EIG_* launch runs (pml_launch.h)
enum PmlOp {
    OP_RESET_ERR, OP_PREP, OP_LOGLIK,
    OP_LEVEL,    // one level launch: entries first .. first + count of the list
    OP_LEVELS,   // several levels in one launch, a workgroup per column: levels first .. first + count of the list's table
    OP_BLOCKS,   // subtree blocks; first = 0: the block schedule's, q + 1: tier q of the thin ends (top-down: the deep bins)
    OP_SUPER, OP_STACK,   // every two-level unit; the stacked units of level / depth `first`
    OP_ROOTS,
    OP_EIG_TIPS, OP_EIG_LEVEL, OP_EIG_NARROW, OP_EIG_TIER,   // eigen models (level: entries; narrow: levels; tier `first`)
    OP_BT_NARROW, OP_BT_TIER, OP_BT_LEVEL,                   // joint back-trace, the same
    OP_COUNT
};
// which unit / node list a launch walks (pml_ctx::d_unit_lists).  The _SORTED lists are sorted by shape inside every level.
enum PmlList {
    L_NONE, L_BU_FUSED, L_BU_FUSED_SORTED, L_TD_FUSED, L_TD_FUSED_SORTED, L_BU_PLAIN, L_TD_PLAIN, L_CHERRIES, L_TOP_BU, L_TOP_TD,
    L_REST_BU, L_REST_BU_SORTED, L_REST_TD, L_REST_TD_SORTED, L_CHILD_UNITS, L_STACK_CHILDREN,
    L_IDS,   // a contiguous range of node ids (the nodes of a depth)
    L_COUNT
};
enum PmlBranch {
    BU_ONE_LAUNCH, BU_BLOCKS, BU_SUPER, BU_THIN, BU_FUSED, BU_FUSED_JOINT, BU_EIGJ_TIERS, BU_EIGJ, BU_GEMM_TIERS, BU_GEMM,
    BU_EIG_FUSED, BU_PLAIN, TD_ONE_LAUNCH, TD_BLOCKS, TD_SUPER, TD_GEMM, TD_EIG_FUSED, TD_DEEP, TD_LEVELS, BT_TIERS, BT_LEVELS,
    PML_BRANCH_COUNT
};
#define PML_NO_BRACKET 255
struct PmlLaunch {
    unsigned char op, list, kind;   // PmlOp, PmlList, SweepKind (OP_EIG_*: PmlEigenFamily)
    unsigned char bracket;          // profile bracket (pml_profile_read's `which`) the launch is counted in, or PML_NO_BRACKET
    unsigned char branch;           // the schedule branch that planned it (for the plan's reader and the tests; not executed)
    bool signal;                    // raises the completion word (the last launch of its sweep)
    bool cherries;                  // top-down staging hint: some unit has a cherry among its first two children
    int first, count;
    int arg;                        // OP_LEVELS: 1 = with the per-branch prep (bottom-up) / the roots are done (top-down); OP_RESET_ERR: 1 = eigen joint;
                                    // OP_SUPER, top-down: d + 1 = the launch also runs the stacked units of depth d (PmlSweepTraits::td_chain), 0 = none
                                    // OP_SUPER, bottom-up: l + 1 = the launch also runs the stacked units of level l (PmlSweepTraits::bu_chain), 0 = none
};
// What an enqueued launch sequence leaves behind for the host that waits for it and reads its results.  A captured graph keeps
// the outcome of what it holds (pml_ctx::GraphSlot): a replay runs none of the code that enqueued it.
struct PmlSweepOutcome {
    int n_signals = 0;           // launches that raise the completion word
    bool final_signals = false;  // the sequence's end raises it
    bool has_params = false;     // the copy of the parameter block is part of the (captured) sequence
    bool fused_joint = false;    // the bottom-up sweep ran the cherry-fused joint branch: the cherries are not in memory
    // this sequence followed by `next` on the same stream
    void then(const PmlSweepOutcome& next) {
        n_signals += next.n_signals;
        final_signals = next.final_signals;
        has_params = has_params || next.has_params;
        fused_joint = fused_joint || next.fused_joint;
    }
};
// Everything the planners read besides the forest and its schedules; filled from a context by sweep_traits (pml_api.hip).
struct PmlSweepTraits {
    bool f81, eigen_fused, eigen_gemm, eigen_joint_valu, hky_fused, wide_states;   // model kind and path
    int k, W, C, sched_cols, n_roots, n_cherries;
    bool has_init, fuse;
    int Gf, Gt;
    bool bu_wide_lanes, level_lists_sorted;   // (these four: copies of the PmlColumnPlan's, pml_columns.h)
    bool single_launch, blocks, super, thin, deep;   // single_launch_sweeps, block_schedule, super_sweeps, thin_bottom_up, deep_top_down
    int narrow_units;                                // NARROW_UNITS (0: not set)
    bool no_td_tail, no_eigg_tiers, no_spin_wait;
    int waves, eig_nb;                               // PML_WAVES_PER_BLOCK, EigShape::NB
    bool td_chain;   // the stacked units of PmlSuperSchedule::chain_depth run inside the top-down two-level launch
    bool bu_chain;   // the stacked units of PmlSuperSchedule::bu_chain_level run inside the bottom-up two-level launch
};
struct PmlSchedules {
    const PmlBlockSchedule* blocks;
    const PmlThinSchedule* thin;
    const PmlDeepSchedule* deep;
    const PmlSuperSchedule* sup;
    const PmlEigenTiers* eig;
    const PmlBacktraceTiers* bt;
    const std::vector<char>*bu_level_vec_f, *bu_level_vec;
    const std::vector<int>* td_cherry_prefix;
};

#define PML_PLAN __attribute__((visibility("hidden")))   // (internal to the library, like pml_host.h's PML_INTERNAL)
// "" when the arrays describe a forest the kernels can index safely, else the reason
PML_PLAN std::string pml_check_tree(const PmlTreeArrays& t);
// the library's numbering of a checked forest and the forest in it; t is pointed at num's arrays when the numbering changes
PML_PLAN PmlForest pml_plan_forest(PmlTreeArrays& t, const PmlTune& tune, bool fuse, PmlNumbering& num);
// t: the arrays in the library's numbering (as pml_plan_forest left them)
PML_PLAN PmlTreePlan pml_plan_tree(const PmlForest& f, const PmlTreeArrays& t, const PmlTune& tune);
// thin: the most units a thin level holds
PML_PLAN PmlThinPlan pml_plan_thin_ends(const PmlForest& f, const PmlTune& tune, int thin);
// the launches of a sweep, in the order they are issued (wants_signal: the pass waits on the top-down sweep's completion word;
// head: the narrow depths below the roots, which decide whether the back-trace replays as a graph)
PML_PLAN std::vector<PmlLaunch> pml_plan_bottom_up(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, bool is_marginal);
PML_PLAN std::vector<PmlLaunch> pml_plan_top_down(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, bool wants_signal);
PML_PLAN std::vector<PmlLaunch> pml_plan_backtrace(const PmlForest& f, const PmlSchedules& s, const PmlSweepTraits& t, int* head);
// the part of a plan's outcome the plan decides (has_params is the enqueuer's)
PML_PLAN PmlSweepOutcome pml_plan_outcome(const std::vector<PmlLaunch>& plan);
