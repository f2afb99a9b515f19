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
