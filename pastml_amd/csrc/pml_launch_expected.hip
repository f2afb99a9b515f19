// Launches of the exact expected transition counts (pml_kernels_expected.h): the branch pass, the pass over the parents and
// the sum of the partials, for the columns [cb, ce) of the context in one go.  pml_expected_counts (pml_api_readers.hip) checks the
// arguments, makes sure every vector the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_expected.h"

// Ids per piece: fixed by k and the model kind, never by the grid (the sums' order, hence their bits, follows from it).
// F81 family: a piece's partial (k^2 doubles) against what its branches stream in (2 k doubles each): 2048 ids keep the partials
// under 2 % of the traffic at k = 64, 4096 under 7 % at k = 512.  Matrix models read k^2 doubles per branch: 128 ids, < 1 %.
static int expected_piece(const pml_ctx* ctx) {
    if (ctx->kind != PML_MODEL_F81) return 128;
    return ctx->k <= 64 ? 2048 : 4096;
}
#define PML_EXP_PARENT_PIECE 4096

// d_alt: [N] in the library's numbering or null; d_out [cols][k][k]; d_same [cols][N][k] (caller's numbering, zeroed) or null
PML_INTERNAL int launch_expected(pml_ctx* ctx, int cb, int ce, const unsigned char* d_alt, double* d_out, double* d_same) {
    const int k = ctx->k, N = ctx->N, cols = ce - cb;
    const bool f81 = ctx->kind == PML_MODEL_F81;
    const bool windowed = pij_windowed(ctx);
    std::vector<int> ids;   // (windowed: the branch list of the call; before the scope, whose copy reads it)
    PmlExpArgs a;
    a.parent = ctx->d_parent;
    a.first_child = ctx->d_first_child;
    a.n_children = ctx->d_n_children;
    a.new_of_old = ctx->d_new_of_old;   // (null when the library works in the caller's numbering)
    a.altered = d_alt;
    a.masks = ctx->d_masks;
    a.pi = ctx->d_pi;
    a.bu = ctx->d_bu;
    a.post = ctx->d_post;
    a.E = f81 ? ctx->d_E : nullptr;
    a.P = f81 ? nullptr : ctx->d_P;
    a.N = N;
    a.k = k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.col0 = cb;
    a.piece = expected_piece(ctx);
    a.n_pieces = (N + a.piece - 1) / a.piece;
    a.ppiece = PML_EXP_PARENT_PIECE;
    a.n_ppieces = (N + a.ppiece - 1) / a.ppiece;
    a.same = d_same;
    a.out = d_out;
    a.partial = a.corr = a.rowsum = a.dterm = nullptr;
    a.piece0 = 0;
    a.win_B = 0;
    const size_t n_partial = (size_t)cols * a.n_pieces * k * k, n_corr = (size_t)cols * a.n_ppieces * k;
    const size_t n_branch = f81 ? (size_t)cols * N : (size_t)cols * N * k;
    CallScope mem(ctx->stream, false);
    double* scratch;   // one allocation: the partials, the parents' corrections, the per-branch terms
    PML_TRY(mem.get(&scratch, n_partial + n_corr + n_branch));
    a.partial = scratch;
    a.corr = scratch + n_partial;
    (f81 ? a.rowsum : a.dterm) = scratch + n_partial + n_corr;
    if (f81) {
        const int T = (k + 15) / 16, TG = (T + 3) / 4;
        if (TG == 1) {
            hipLaunchKernelGGL(expected_f81_kernel<0>, dim3(a.n_pieces, 1, cols), dim3(256), 0, ctx->stream, a);
        } else {
            hipLaunchKernelGGL(expected_rowsum_kernel, dim3((N + 15) / 16, cols), dim3(256), 0, ctx->stream, a);
            hipLaunchKernelGGL(expected_f81_kernel<1>, dim3(a.n_pieces, TG * TG, cols), dim3(256), 0, ctx->stream, a);
        }
    } else if (windowed) {
        // P(t) in a window: runs of whole pieces, each behind the build of its ids' branches for the columns of the call (the x
        // range of the grid starts at the run's first piece: partials, per-branch terms and the reduce do not notice).  A window
        // below one piece: the call takes one of a piece per column of its own, gone with the scope.
        if (k > 256) return fail(PML_ERR_UNSUPPORTED, "k = %d: the matrix models hold at most 256 states", k);
        double* window = ctx->d_pij_window;
        a.win_B = ctx->pij_window;
        if (a.win_B < a.piece) {
            a.win_B = a.piece;
            PML_TRY(mem.get(&window, (size_t)cols * a.piece * k * ctx->ks));
        }
        a.P = window;
        std::vector<PmlPieceRun> runs;
        const std::string bad = pml_window_piece_runs(N, a.piece, a.win_B, runs);
        if (!bad.empty()) return fail(PML_ERR_INVALID, "%s", bad.c_str());
        ids.resize((size_t)N);
        for (int i = 0; i < N; ++i) ids[(size_t)i] = ctx->new_of_old.empty() ? i : ctx->new_of_old[(size_t)i];
        int* d_ids;
        PML_TRY(mem.put(&d_ids, (const int*)ids.data(), ids.size()));
        const int rows = k <= 64 ? 1 : (k <= 128 ? (k + 63) / 64 : (k + 31) / 32);
        for (const PmlPieceRun& r : runs) {
            const int i0 = r.p0 * a.piece, i1 = std::min(N, r.p1 * a.piece);
            PML_TRY(launch_pij_wide_list(ctx, window, a.win_B, d_ids + i0, i1 - i0, cb, ce));   // (a root among them: built, never read)
            a.piece0 = r.p0;
            const dim3 grid(r.p1 - r.p0, rows, cols);
            if (k <= 64) hipLaunchKernelGGL((expected_matrix_kernel<1, true>), grid, dim3(256), 0, ctx->stream, a);
            else if (k <= 128) hipLaunchKernelGGL((expected_matrix_kernel<2, true>), grid, dim3(256), 0, ctx->stream, a);
            else hipLaunchKernelGGL((expected_matrix_kernel<4, true>), grid, dim3(256), 0, ctx->stream, a);
        }
        a.piece0 = 0;
    } else if (k <= 64) {
        hipLaunchKernelGGL(expected_matrix_kernel<1>, dim3(a.n_pieces, 1, cols), dim3(256), 0, ctx->stream, a);
    } else if (k <= 128) {
        hipLaunchKernelGGL(expected_matrix_kernel<2>, dim3(a.n_pieces, (k + 63) / 64, cols), dim3(256), 0, ctx->stream, a);
    } else if (k <= 256) {
        hipLaunchKernelGGL(expected_matrix_kernel<4>, dim3(a.n_pieces, (k + 31) / 32, cols), dim3(256), 0, ctx->stream, a);
    } else {
        return fail(PML_ERR_UNSUPPORTED, "k = %d: the matrix models hold at most 256 states", k);
    }
    hipLaunchKernelGGL(expected_parents_kernel, dim3(a.n_ppieces, cols), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(expected_reduce_kernel, dim3((k * k + 255) / 256, cols), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return mem.finish();   // (the scratch goes)
}
