// P(t) of the eigen models beyond 32 states in a window instead of a batch of the whole tree: a finished sweep plan of plain
// level launches (BU_PLAIN / TD_LEVELS, pml_schedule.h) cut into runs of parents whose children's matrices fit a window of B
// branches.  A run is one level launch over its parents, preceded by one launch that builds exactly its children's matrices
// into the window (pml_kernels_pij_wide.h, the list form); the stream orders the build of run n + 1 behind the sweep launch of
// run n, so one buffer serves a whole sweep.  Every matrix is computed by the instructions that compute it for the batch --
// only its address changes --, so a windowed sweep leaves the bits of a materialised one.
//   * a parent's children are never split over two runs, so B is at least the largest fan-out of the forest;
//   * a run never crosses a level boundary (a level reads what the level before it wrote);
//   * every other record of the plan (error reset, the per-branch pass, ln L, the roots, the completion signal) keeps its
//     place; the per-branch pass builds nothing in window mode (run_plan skips it).
// Plain C++ over plain tables, like pml_schedule.h: built, tested and sanitised on any host (tests/pij_window_plan_driver.cpp).
#pragma once
#include "pml_schedule.h"

// A record of the windowed sequence: a record of the plan (a level record possibly cut down to a run of its parents) and the
// branches whose matrices are built into the window before it.
struct PmlWindowStep {
    PmlLaunch launch;
    int build_first, build_count;   // entries [build_first, build_first + build_count) of `branches` into slots 0 .. build_count - 1
};
struct PmlWindowPlan {
    std::vector<PmlWindowStep> steps;
    std::vector<int> branches;   // child ids in run order (every branch some level record of the plan reads, once)
    std::vector<int> slot;       // per node: its slot in the window of the run that reads its branch, -1 where no run does
    int runs = 0;                // runs that build something
};

// the largest number of children of a node
PML_PLAN int pml_window_max_fanout(const PmlForest& f);
// bu_order / td_parents: the node lists the plan's L_BU_PLAIN / L_TD_PLAIN level records index (pml_tree_upload's arrays in the
// library's numbering).  "" and the windowed sequence in `out`, else the reason (B below the largest fan-out, a record beyond
// its list).
PML_PLAN std::string pml_plan_pij_window(const std::vector<PmlLaunch>& plan, const PmlForest& f, const std::vector<int>& bu_order,
                                         const std::vector<int>& td_parents, long long B, PmlWindowPlan& out);

// ---- the consumers of P(t) outside the sweeps: the exact and the sampled counts, the simulator, the scenario sampler ----------
// They run in runs as well: one launch of the list build for exactly the branches the next consumer launch reads (for the
// columns of the call only), then that launch, which finds branch i of the run's list in slot i.  The sampled counts walk the
// top-down level list and take the runs of the top-down sweep (PmlWindowPlan above, kept on the context); the cuts of the other
// three are below.  None of them moves a floating-point sum or a draw: a run only says where a matrix lies.

// Exact counts: the branch pass walks the caller's ids in pieces of `piece`, one workgroup per piece; a run is the whole pieces
// [p0, p1), its branch list the ids [piece p0, min(n_ids, piece p1)) in order (slot = id - piece p0).  B < piece: refused -- the
// call then takes a window of one piece of its own.
struct PmlPieceRun {
    int p0, p1;
};
PML_PLAN std::string pml_window_piece_runs(int n_ids, int piece, long long B, std::vector<PmlPieceRun>& out);

// Simulator and scenario sampler (pml_launch_simulate.hip): the depth levels above the frontier one launch per run of at most B
// consecutive nodes (slot = node - first node of the run; depth 0 are the roots and builds nothing), the subtrees rooted at the
// frontier depth in groups of consecutive subtrees whose preorder lists hold at most B entries together (slot = position in the
// group; a root among them is built harmlessly and never read).  A subtree is never split: where one at the asked depth holds
// more than B nodes the frontier moves down for this call -- in the limit to the number of levels, level launches only.  The
// results cannot tell: a node's draw is a function of (seed, node, repetition).
struct PmlSimWindowRun {
    int first, count;               // a level run: nodes; a group: frontier subtrees (indices into sub_off)
    int build_first, build_count;   // entries of `order` built into slots 0 .. build_count - 1 (0: nothing)
};
struct PmlSimWindowPlan {
    int depth = 0;                  // the frontier depth used (>= the one asked for)
    std::vector<PmlSimWindowRun> levels, groups;
    std::vector<int> order;         // the branch lists of the runs one after the other, then the subtrees in preorder
    int list_base = 0;              // where the subtrees begin in `order`
    std::vector<int> sub_off;       // [subtrees + 1]: a subtree's entries, counted from list_base
};
PML_PLAN std::string pml_plan_sim_window(const PmlForest& f, int depth, long long B, PmlSimWindowPlan& out);
