// The column layout, planned on the host: everything pml_chars_alloc decides from the number of columns, the number of states
// and the forest before it allocates -- the padded row, the lane shapes of the matrix and the F81 kernels, which lists the level
// launches walk, whether the levels fit a workgroup, where the thin ends are cut, and the layout of the parameter block.  Plain
// C++ like pml_schedule.h: no HIP, so that the rules that decide a column's bits can be built, tested and sanitised on any host.
#pragma once
#include <cstddef>
#include <string>

#include "pml_schedule.h"

#define PML_COLUMNS_MAX_STATES 512   // (PML_MAX_STATES of the kernels; pml_api.hip asserts that they agree)

// pi, sf, tau, tau factor, mu, kappa of all columns live in ONE device block with a pinned host mirror of the same layout
// (pml_ctx::d_params / h_params); behind them the flags of the active columns and, last, one word for the top-down sweep: the
// observed tips' rows are kept.  Element offsets into either; pi is [C][ks], the others [C], keep_tips one word.
struct PmlParamBlock {
    size_t pi = 0, sf = 0, tau = 0, tauf = 0, mu = 0, kappa = 0, active = 0, keep_tips = 0;
    size_t count = 0;   // elements of the whole block
    // an array of the block behind `base` (d_params or h_params; null while the columns are not allocated)
    template <class T>
    static T* at(T* base, size_t offset) { return base ? base + offset : nullptr; }
};

struct PmlLaneShape {
    int g, r;   // lanes per unit, states per lane
};

// lanes per unit of PmlColumnPlan::bu_shape for those who hold copies of the plan's two fields (PmlSweepTraits: the planners of
// the sweeps' launches, pml_schedule.cpp)
static inline int pml_bu_lanes(bool bu_wide_lanes, int Gf) { return bu_wide_lanes ? 8 : Gf; }

struct PmlColumnPlan {
    int C = 0, k = 0;
    int ks = 0;   // states of a padded row: a multiple of the matrix kernels' R, even from two states on (16-byte lane accesses)
    int W = 0;    // mask words per node
    int G = 0, R = 0;     // lane group of the matrix kernels
    int Gf = 0, Rf = 0;   // lane-group shape of the F81-family bottom-up kernels (chunked state ownership)
    int Gt = 0, Rt = 0;   // ... and of the F81-family top-down kernels
    bool bu_wide_lanes = false;         // 32 < k <= 64: most bottom-up levels run with 8 states per lane (dispatch_sweep_f81)
    bool level_lists_sorted = false;    // the level launches walk the lists sorted by shape (pml_plan_tree)
    bool levels_fit_workgroup = false;  // (nearly) every fused level is one pass of a PML_SMALL_BLOCK-thread workgroup
    int thin_units = 0;                 // the most units a thin level holds (pml_plan_thin_ends); 0: no thin ends are built
    PmlParamBlock params;

    // Lane shape of the bottom-up launches that do not stream stored vectors: the kernels that walk several levels in one
    // launch, the two-level and the stacked units.  It is the shape the level kernels use for levels of that size
    // (dispatch_sweep_f81: 8 states per lane up to 65 536 units when 32 < k <= 64).  The reductions over a unit's lanes associate
    // differently in different shapes, so a level must get the same shape whether it runs there or in a level launch: where
    // the narrow end begins depends on the number of columns, and a column's bits must not.
    PmlLaneShape bu_shape() const { return {pml_bu_lanes(bu_wide_lanes, Gf), bu_wide_lanes ? 8 : Rf}; }
    PmlLaneShape td_shape() const { return {Gt, Rt}; }
    PmlLaneShape shape(bool bottom_up) const { return bottom_up ? bu_shape() : td_shape(); }
};

// "" and the plan in `out`, or the reason why n_cols columns of k states cannot be laid out on this forest (`out` untouched)
PML_PLAN std::string pml_plan_columns(const PmlForest& f, const PmlTune& tune, int n_cols, int k, PmlColumnPlan& out);
