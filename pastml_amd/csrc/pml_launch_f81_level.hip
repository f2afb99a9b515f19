// Launchers of the F81-family level kernels (one launch per fused height / depth).
#include "pml_launch_f81_level.h"

int dispatch_sweep_f81(pml_ctx* ctx, SweepKind what, const PmlUnit* units, int n_level, bool cherries, bool bu_sweep) {
    if (n_level <= 0) return PML_OK;
    if (what == SW_TD) return fail(PML_ERR_INVALID, "the F81 kernels walk descriptor lists: SW_TD has none");
    const bool td = what == SW_TD_FUSED || what == SW_ROOTS;
    const PmlColumnPlan& cols = ctx->cols;
    // Fused bottom-up levels, 32 < k <= 64 (measured on cfg4): 8 states per lane (8 units per wavefront share the
    // per-unit scalar work) wins on the level that rebuilds cherries (1.80 -> 1.58 ms) and on small levels;
    // 4 states per lane (twice the loads in flight per unit) wins on big levels that stream stored vectors.
    // (SW_BU_CHERRIES rewrites pi . v of the cherries, which the level that rebuilds them has stored: same shape, or
    // a download of the bottom-up vectors would change the last bit of what a later top-down sweep reads)
    const bool wide_lanes = what == SW_BU_MARG_FUSED_NOVEC || what == SW_BU_CHERRIES || (what == SW_BU_MARG_FUSED && n_level <= 65536);
    const auto [g, r] = td ? cols.td_shape() : (wide_lanes ? cols.bu_shape() : PmlLaneShape{cols.Gf, cols.Rf});
#define X(G_, R_)                                                \
if (g == G_ && r == R_) {                                    \
    launch_sweep_f81<G_, R_>(ctx, what, units, n_level, cherries, bu_sweep);     \
    HIP_TRY(hipGetLastError());                              \
    return PML_OK;                                           \
}
    PML_F81_CASES(X)
#undef X
    if (g == 64 && r == 8) return dispatch_sweep_f81_wide(ctx, what, units, n_level, cherries, bu_sweep);   // (more than 256 states)
    return fail(PML_ERR_UNSUPPORTED, "no F81 kernel for G=%d R=%d", g, r);
}
