// Launchers of the two-level and stacked units of the F81-family sweeps (pml_kernels_f81.h).
#include "pml_launch.h"

template <int G, int R, bool LANES, bool PIPE>
static void launch_td_super_f81(pml_ctx* ctx, dim3 grid, const PmlTree& t, const PmlCols& c, const PmlState& st) {
    hipLaunchKernelGGL((td_f81_super_kernel<G, R, LANES, PIPE>), grid, dim3(PML_BLOCK), 0, ctx->stream, t, c, st, ctx->sup.d_units,
                       ctx->sup.n);
}

// The chained top-down launch (td_f81_chain_kernel): the stacked units of depth chain_depth, n of them from entry a of the
// top-down stacked list, and the two-level units below them.  A wave's unit of work is a tile, one pass of stacked child-units
// and four of two-level child-units, on the grid of the pipelined kernels.
template <int G, int R>
static void launch_td_chain_f81(pml_ctx* ctx, int a, const PmlTree& t, const PmlCols& c, const PmlState& st) {
    const int tiles = (2 * ctx->sup.n + 4 * (64 / G) - 1) / (4 * (64 / G));
    dim3 grid(grid_for(ctx, tiles, PML_WAVES_PER_BLOCK, ctx->C, true), ctx->C);
    if (!ctx->tune.on(T_NO_TIP_LANES))
        hipLaunchKernelGGL((td_f81_chain_kernel<G, R, true>), grid, dim3(PML_BLOCK), 0, ctx->stream, t, c, st, ctx->sup.d_units,
                           ctx->sup.n, ctx->sup.d_stack_td + a);
    else
        hipLaunchKernelGGL((td_f81_chain_kernel<G, R, false>), grid, dim3(PML_BLOCK), 0, ctx->stream, t, c, st, ctx->sup.d_units,
                           ctx->sup.n, ctx->sup.d_stack_td + a);
}

// The chained bottom-up launch (bu_f81_chain_kernel): the two-level units and the stacked units of level bu_chain_level above
// them, n / 4 of them from entry a of the bottom-up stacked list.  A wave's unit of work is a tile, four passes of two-level
// units and one of stacked units, on the grid of the pipelined kernels.
template <int G, int R>
static void launch_bu_chain_f81(pml_ctx* ctx, int a, const PmlTree& t, const PmlCols& c, const PmlState& st) {
    const int tiles = (ctx->sup.n + 4 * (64 / G) - 1) / (4 * (64 / G));
    dim3 grid(grid_for(ctx, tiles, PML_BU_CHAIN_WAVES, ctx->C, true), ctx->C);
    hipLaunchKernelGGL((bu_f81_chain_kernel<G, R>), grid, dim3(64 * PML_BU_CHAIN_WAVES), 0, ctx->stream, t, c, st, ctx->sup.d_units,
                       ctx->sup.n, ctx->sup.d_stack_bu + a);
}

template <int G, int R>
static void launch_super_f81(pml_ctx* ctx, bool bottom_up, int chain_first) {
    const PmlTree t = tree_of(ctx, true);
    const PmlCols c = cols_of(ctx, bottom_up);
    const PmlState st = state_of(ctx);
    if (chain_first >= 0 && bottom_up) return launch_bu_chain_f81<G, R>(ctx, chain_first, t, c, st);
    if (chain_first >= 0) return launch_td_chain_f81<G, R>(ctx, chain_first, t, c, st);
    const int upb = PML_WAVES_PER_BLOCK * (64 / G);
    // Top-down: one unit per child of a two-level node.  Every lane shape loads one unit ahead (td_f81_super_kernel's PIPE,
    // profiles/td_super_pipeline.txt) and then likes the grid of the pipelined bottom-up kernels.
    const bool pipe = bottom_up || !ctx->tune.on(T_NO_TD_SUPER_PIPE);
    dim3 grid(grid_for(ctx, bottom_up ? ctx->sup.n : 2 * ctx->sup.n, upb, ctx->C, pipe), ctx->C), block(PML_BLOCK);
    const bool lanes = !ctx->tune.on(T_NO_TIP_LANES);  // the four observed tips of a unit finished in lanes (pml_kernels_f81.h)
    if (bottom_up)
        hipLaunchKernelGGL((bu_f81_super_kernel<G, R>), grid, block, 0, ctx->stream, t, c, st, ctx->sup.d_units, ctx->sup.n);
    else if (pipe && lanes)
        launch_td_super_f81<G, R, true, true>(ctx, grid, t, c, st);
    else if (pipe)
        launch_td_super_f81<G, R, false, true>(ctx, grid, t, c, st);
    else if (lanes)
        launch_td_super_f81<G, R, true, false>(ctx, grid, t, c, st);
    else
        launch_td_super_f81<G, R, false, false>(ctx, grid, t, c, st);
}

// stacked units of bottom-up level / depth `level` (pml_kernels_f81.h)
template <int G, int R>
static void launch_stack_f81(pml_ctx* ctx, bool bottom_up, int a, int n) {
    const PmlTree t = tree_of(ctx, true);
    const PmlCols c = cols_of(ctx, bottom_up);
    const PmlState st = state_of(ctx);
    const int upb = PML_WAVES_PER_BLOCK * (64 / G);
    dim3 grid(grid_for(ctx, bottom_up ? n : 2 * n, upb, ctx->C), ctx->C), block(PML_BLOCK);
    if (bottom_up)
        hipLaunchKernelGGL((bu_f81_stack_kernel<G, R>), grid, block, 0, ctx->stream, t, c, st, ctx->sup.d_stack_bu + a, n);
    else
        hipLaunchKernelGGL((td_f81_stack_kernel<G, R>), grid, block, 0, ctx->stream, t, c, st, ctx->sup.d_stack_td + a, n);
}

int dispatch_super_f81(pml_ctx* ctx, bool bottom_up, int chain) {
    if (ctx->sup.n <= 0) return PML_OK;  // (a schedule of stacked units only)
    int chain_first = -1;
    if (chain >= 0) {
        // (the planner chains a depth or a level only when its stacked range covers the two-level list: pml_plan_tree)
        const std::vector<int>& off = bottom_up ? ctx->sup.stack_bu_offsets : ctx->sup.stack_td_offsets;
        if (chain != (bottom_up ? ctx->sup.bu_chain_level : ctx->sup.chain_depth) || chain + 1 >= (int)off.size() ||
            (long long)(off[chain + 1] - off[chain]) * 4 != ctx->sup.n)
            return fail(PML_ERR_INVALID, "no chained two-level launch for %s %d", bottom_up ? "level" : "depth", chain);
        chain_first = off[chain];
    }
    const auto [g, r] = ctx->cols.shape(bottom_up);
#define X(G_, R_)                                                \
    if (g == G_ && r == R_) {                                    \
        launch_super_f81<G_, R_>(ctx, bottom_up, chain_first);   \
        HIP_TRY(hipGetLastError());                              \
        return PML_OK;                                           \
    }
    PML_SUPER_CASES(X)
#undef X
    return fail(PML_ERR_UNSUPPORTED, "no two-level F81 kernel for G=%d R=%d", g, r);
}

int dispatch_stack_f81(pml_ctx* ctx, bool bottom_up, int level) {
    const std::vector<int>& off = bottom_up ? ctx->sup.stack_bu_offsets : ctx->sup.stack_td_offsets;
    if (ctx->sup.n_stack == 0 || level + 1 >= (int)off.size()) return PML_OK;
    const int a = off[level], n = off[level + 1] - a;
    if (n <= 0) return PML_OK;
    const auto [g, r] = ctx->cols.shape(bottom_up);
#define X(G_, R_)                                         \
    if (g == G_ && r == R_) {                             \
        launch_stack_f81<G_, R_>(ctx, bottom_up, a, n);   \
        HIP_TRY(hipGetLastError());                       \
        return PML_OK;                                    \
    }
    PML_SUPER_CASES(X)
#undef X
    return fail(PML_ERR_UNSUPPORTED, "no stacked F81 kernel for G=%d R=%d", g, r);
}

