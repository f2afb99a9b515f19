// The column layout's planner (pml_columns.h).  Plain C++, no HIP.
#include "pml_columns.h"

#include <algorithm>

// the fewest lanes, a power of two, that hold k states at r states per lane
static int lanes_for(int k, int r) {
    const int need = (k + r - 1) / r;
    int g = 1;
    while (g < need) g <<= 1;
    return g;
}

// pi, sf, tau, tau factor, mu, kappa, active; the observed tips' rows are kept
static PmlParamBlock param_block(size_t C, size_t ks) {
    PmlParamBlock b;
    b.pi = 0;
    b.sf = b.pi + C * ks;
    b.tau = b.sf + C;
    b.tauf = b.tau + C;
    b.mu = b.tauf + C;
    b.kappa = b.mu + C;
    b.active = b.kappa + C;
    b.keep_tips = b.active + C;
    b.count = b.keep_tips + 1;
    return b;
}

std::string pml_plan_columns(const PmlForest& f, const PmlTune& tune, int n_cols, int k, PmlColumnPlan& out) {
    if (n_cols <= 0 || n_cols > 65535) return "n_cols must be in 1..65535";
    if (k <= 0) return "k must be positive";
    if (k > PML_COLUMNS_MAX_STATES)
        return "k = " + std::to_string(k) + " states; at most " + std::to_string(PML_COLUMNS_MAX_STATES) + " are supported";
    PmlColumnPlan p;
    p.C = n_cols;
    p.k = k;
    // lane group of the matrix kernels
    p.R = k <= 32 ? 1 : (k <= 128 ? 2 : (k <= 256 ? 4 : 8));   // (beyond 256 states: the F81 family only, a wavefront per unit)
    if (k > 16 && k <= 32) p.R = 4;  // 8 lanes per unit: 8 units per wavefront
    p.G = lanes_for(k, p.R);
    p.ks = (k + p.R - 1) / p.R * p.R;
    // F81 family: 4 states per lane (two 16-byte pairs).  Most of a unit's work is scalar (per child, per tip), so
    // the top-down kernels, which have the most of it, take 8 states per lane for 32 < k <= 64: 8 units per
    // wavefront share each scalar instruction.  PASTML_HIP_F81_R / PASTML_HIP_F81_TD_R = 2 / 4 / 8: tuning variants
    // Forests with many nodes of three or four children (15 % of the nodes with grandchildren) take 16 lanes per unit where
    // k allows it: the lane-parallel gather of a unit's children (Gather<G>) takes G / 4 of them -- two with 8 lanes, four
    // with 16 --, a unit with more walks them one after the other and holds up the other units of its wavefront.
    const bool polytomies = f.polytomies;
    auto shape = [&](int var, int dflt, int& G, int& R) {
        int rf = k >= 3 ? dflt : k;
        // Up to 8 states: two per lane (2 or 4 lanes per unit).  In the latency-bound schedules -- small and mid-size
        // forests -- a level is one wavefront's instruction stream, and half the states per lane are a shorter one
        // (HIV1C tree, 14 columns: bottom-up sweep k = 4 0.111 -> 0.094 ms, k = 8 0.107 -> 0.095; marginal pass
        // 0.290 -> 0.262, 0.319 -> 0.262; cfg2 0.0765 -> 0.0713 ms); the level kernels of large forests are
        // indifferent (262 144 tips x 32 characters, k = 4: balanced 0.73 -> 0.77 ms, ragged 2.46 -> 2.34).  One state
        // per lane is another 3 - 5 % on the small forests and costs the large balanced one a third: not taken.
        if (k >= 3 && k <= 8 && dflt == 4) rf = 2;
        // 16 < k <= 32 on forests with polytomies: 16 lanes x 2 states instead of 8 x 4 (100 000 tips, at most 3 children, x 16
        // columns, k = 20 / 32: marginal pass 1.33 -> 0.95 / 1.34 -> 0.96 ms; at most 5 children: no change; binary trees lose 6 %)
        if (k > 16 && k <= 32 && dflt == 4 && polytomies) rf = 2;
        if (tune.on(var)) {
            const int v = (int)tune.get(var, 0);
            if ((v == 2 || v == 4 || v == 8) && k > 32 && k <= 64) rf = v;
            if ((v == 2 || v == 4) && k >= 3 && k <= 8) rf = v;
            if ((v == 2 || v == 4) && k > 16 && k <= 32) rf = v;   // (16 lanes x 2 states or 8 x 4)
        }
        if (k > 256) rf = 8;   // (a wavefront per unit: 64 lanes x 8 states, k <= 512)
        R = rf;
        G = lanes_for(k, rf);
    };
    shape(T_F81_R, 4, p.Gf, p.Rf);
    // Balanced parts (PmlForest::balanced_parts): counted on the topology alone, whatever the switches, so that the lane
    // shape, and with it a column's bits, is a function of k and the forest.
    const bool balanced_parts = f.balanced_parts;
    // 8 states per lane bottom-up (32 < k <= 64) where the forest has such parts (cfg4: the level that rebuilds cherries
    // 1.80 -> 1.58 ms; 262 144-tip balanced tree x 32: bottom-up 0.77 -> 0.63 ms) and few nodes of three or four children
    // (8 lanes gather two children in parallel, see below); elsewhere 4: polytomies x 16 columns bottom-up 0.64 -> 0.50 ms
    // (at most 3 children), 0.61 -> 0.52 (at most 5); random binary 40 000 tips x 8 0.184 -> 0.161; 262 144 x 16 1.17 -> 1.13
    // (profiles/r05y_lane_shapes_and_sorted_levels.txt).
    p.bu_wide_lanes = k > 32 && k <= 64 && p.Rf == 4 && !tune.on(T_F81_R) && balanced_parts && !polytomies;
    if (tune.on(T_BU_WIDE)) p.bu_wide_lanes = k > 32 && k <= 64 && p.Rf == 4 && tune.get(T_BU_WIDE, 1) != 0;
    // Level launches walk the lists sorted by shape inside every level (pml_plan_tree) from 4 lanes per unit on: 262 144
    // tips x 32, marginal pass: k = 8 1.82 -> 1.78 ms, k = 12 2.35 -> 2.26, k = 16 2.38 -> 2.26, k = 20 3.49 -> 3.06, k = 32
    // 3.53 -> 3.11; polytomies k = 12 1.36 -> 1.28, k = 20 1.55 -> 1.36; two lanes per unit (k <= 4) lose 11 % and keep id order.
    p.level_lists_sorted = p.Gf >= 4 || f.shape_ordered;   // (narrow units too where the numbering follows the shapes)
    if (tune.on(T_SORT_LEVELS)) p.level_lists_sorted = tune.get(T_SORT_LEVELS, 1) != 0;
    // Top-down: 8 states per lane for 32 < k <= 64 (above) unless the forest has many nodes of three or four children
    // (15 % of those with grandchildren): the lane-parallel gather of a unit's children takes
    // G / 4 of them (Gather<G>::CH: two with 8 lanes, four with 16), a unit with more walks them one after the other and
    // holds up the other units of its wavefront.  Measured, marginal pass, k = 64 (profiles/r05y_lane_shapes_and_sorted_levels.txt):
    // 100 000 tips, at most 3 children per node, x 8 / 16 / 32 columns 1.37 -> 0.93 / 1.79 -> 1.38 / 2.84 -> 2.26 ms; at
    // most 5 children x 16 2.12 -> 1.90; at most 8 2.52 -> 2.28; binary trees lose 5 % with 4 states per lane.  The shape
    // follows k and the forest, never the columns.
    shape(T_F81_TD_R, (k > 32 && k <= 64 && !polytomies) ? 8 : 4, p.Gt, p.Rt);
    if (k >= 2 && (p.ks & 1)) p.ks += 1;  // 16-byte lane accesses
    {
        const int g = p.bu_shape().g;
        const int nl = (int)f.bu_offsets_f.size() - 1;
        long long passes = 0;
        for (int l = 0; l < nl; ++l)
            passes += ((long long)(f.bu_offsets_f[l + 1] - f.bu_offsets_f[l]) * g + PML_SMALL_BLOCK - 1) / PML_SMALL_BLOCK;
        // (up to 4 lanes per unit, k <= 16: with wider units one workgroup per column is too little parallelism --
        // HIV1C tree, 64 columns: k = 12 0.28 against 0.32 ms with level launches, k = 20 0.27 against 0.22)
        p.levels_fit_workgroup = nl > 0 && g <= 4 && passes * 4 <= (long long)nl * 5;
    }
    p.W = (k + 63) / 64;
    // the kernels address one column's slab with 32-bit element offsets
    if ((size_t)f.N * p.ks >= (1ull << 31))
        return "n_nodes * k = " + std::to_string((size_t)f.N * p.ks) + " exceeds 2^31 elements per column";
    p.params = param_block((size_t)n_cols, (size_t)p.ks);
    // Thin ends of a large forest.  A level is thin while a launch of its own is mostly latency: up to 4 096 units, and up to
    // THIN_BYTES (20 MB) of state vectors over all columns -- beyond, the level kernels stream it faster than workgroups
    // that walk subtrees.  Measured (profiles/r05u_thin_ends.txt, THIN_UNITS sweeps): k = 4 x 32 columns 4 096 (16 384 loses
    // 20 %); k = 64: x 32 columns 1 024 - 2 048, x 16 2 048, x 8 4 096; k = 20 x 32 4 096.
    // (more than 256 states run the plain level schedule: no thin ends)
    if (k <= 256 && !f.bu_offsets_f.empty() && (f.bu_offsets_f.back() > 2048 || tune.on(T_THIN_UNITS)) && !tune.on(T_NO_THIN)) {
        long long thin = tune.get(T_THIN_UNITS, 0);
        if (!tune.on(T_THIN_UNITS)) {
            const long long bytes = tune.get(T_THIN_BYTES, 20ll << 20);
            thin = std::min(4096ll, std::max(256ll, bytes / ((long long)n_cols * p.ks * 8)));
        }
        p.thin_units = (int)thin;
    }
    out = p;
    return "";
}
