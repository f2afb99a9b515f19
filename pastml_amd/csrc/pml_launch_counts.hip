// Launches of the scenario sampling of marginal_counts (pml_kernels_counts.h): the roots, then one launch per depth level -- or,
// on a context with a P(t) window, per run of the top-down sweep's window plan.  pml_marginal_counts (pml_api_readers.hip) checks
// the arguments, makes sure every vector the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_counts.h"

PML_INTERNAL int counts_max_states() { return PML_COUNTS_MAX_K; }

// d_alt: [N] in the library's numbering or null (see counts_level_kernel); d_counts [N][k]; d_result [k][k] (zeroed); d_same [N][k]
// (zeroed) or null.  Queued only.
PML_INTERNAL int launch_counts(pml_ctx* ctx, int col, int n_rep, u64 seed, const unsigned char* d_alt, int* d_counts,
                               long long* d_result, int* d_same) {
    const PmlTree t = tree_of(ctx);
    const PmlCols c = cols_of(ctx);
    const PmlState st = state_of(ctx);
    const PmlModel m = model_of(ctx);
    const double* P = ctx->kind == PML_MODEL_F81 ? nullptr : ctx->d_P;
    // (the draws are keyed by the CALLER's node ids: the library's internal numbering must not show in the result)
    hipLaunchKernelGGL(counts_roots_kernel, dim3(std::min(ctx->n_roots, 1024)), dim3(64), 0, ctx->stream, t, c, st, col, n_rep, seed,
                       d_counts, ctx->d_old_of_new);
    if (pij_windowed(ctx)) {
        // the runs of the top-down sweep (parents of one level whose children fit the window), each behind the build of its
        // children's matrices for this column: the draws are keyed by the node, so the cuts do not show
        const PmlPWindow w = {ctx->d_pij_window, ctx->d_win_slot[1], ctx->pij_window};
        size_t covered = 0;
        for (const PmlWindowStep& r : ctx->win_td_runs) covered += (size_t)r.launch.count;
        if (covered != ctx->td_parents.size())
            return fail(PML_ERR_INVALID, "the window's top-down runs cover %zu of %zu parents", covered, ctx->td_parents.size());
        for (const PmlWindowStep& r : ctx->win_td_runs) {
            if (r.build_count > 0)
                PML_TRY(launch_pij_wide_list(ctx, ctx->d_pij_window, ctx->pij_window, ctx->d_win_branches[1] + r.build_first,
                                             r.build_count, col, col + 1));
            hipLaunchKernelGGL(counts_level_kernel<PML_P_WINDOW>, dim3(std::min(r.launch.count, 65536)), dim3(64), 0, ctx->stream,
                               t, c, st, m, w, col, n_rep, seed, ctx->d_td_parents + r.launch.first, r.launch.count, d_counts,
                               d_result, ctx->d_old_of_new, d_alt, d_same);
        }
    } else
    for (int l = 0; l < ctx->n_td_levels; ++l) {
        const int a = ctx->forest.td_parent_offsets[l], b = ctx->forest.td_parent_offsets[l + 1];
        if (b <= a) continue;
        hipLaunchKernelGGL(counts_level_kernel<>, dim3(std::min(b - a, 65536)), dim3(64), 0, ctx->stream, t, c, st, m, P, col, n_rep,
                           seed, ctx->d_td_parents + a, b - a, d_counts, d_result, ctx->d_old_of_new, d_alt, d_same);
    }
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
