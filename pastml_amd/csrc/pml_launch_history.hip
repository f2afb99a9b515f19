// Launches of the exact expected dwell times and Markov jumps of the F81 family (pml_kernels_history.h): the branch pass, the
// jump product and the sums of the partials, for the columns [cb, ce) of the context in one go, queued on the context's stream.
// pml_expected_history (pml_api_readers.hip) checks the arguments, makes sure every vector the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_history.h"

// Ids -- per time interval: segments -- per piece: fixed by k, never by the grid or by the bins (the sums' order, hence their
// bits, follows from it); a segment streams what a branch streams.
// Branch pass: gradient_piece's sizes, for its reasons -- a piece's partial is 2 k doubles against the 2 k doubles EACH of its
// branches streams in, under 1 % of the traffic everywhere, and a single column of a few thousand nodes still spreads over
// several workgroups.
int history_piece(int k) { return k <= 4 ? 1024 : (k <= 64 ? 512 : 256); }
// Jump product: expected_piece's sizes, for its reasons -- a piece's partial (k^2 doubles) against what its branches stream in
// (2 k doubles each): 2048 ids keep the partials under 2 % of the traffic at k = 64, 4096 under 7 % at k = 512.
int history_jump_piece(int k) { return k <= 64 ? 2048 : 4096; }

void history_args(const pml_ctx* ctx, int cb, PmlHistArgs& a) {
    a = PmlHistArgs{};   // (the pieces, the scratch and the outputs: the caller's)
    a.parent = ctx->d_parent;
    a.n_children = ctx->d_n_children;
    a.new_of_old = ctx->d_new_of_old;   // (null when the library works in the caller's numbering)
    a.dist = ctx->d_dist;
    a.masks = ctx->d_masks;
    a.pi = ctx->d_pi;
    a.bu = ctx->d_bu;
    a.post = ctx->d_post;
    a.E = ctx->d_E;
    a.mu = ctx->d_mu;
    a.sf = ctx->d_sf;
    a.tau = ctx->d_tau;
    a.tauf = ctx->d_tauf;
    a.N = ctx->N;
    a.k = ctx->k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.col0 = cb;
}

// d_times [cols][k]; d_jumps [cols][k][k] or null; d_branch [cols][N] (caller's numbering) or null.  Queued only: partials and
// staged scalars live in the caller's scope, which makes the call's one wait.
PML_INTERNAL int launch_history(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_times, double* d_jumps, double* d_branch) {
    const int k = ctx->k, N = ctx->N, cols = ce - cb;
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    PmlHistArgs a;
    history_args(ctx, cb, a);
    a.piece = history_piece(k);
    a.n_pieces = (N + a.piece - 1) / a.piece;
    a.jpiece = history_jump_piece(k);
    a.n_jpieces = (N + a.jpiece - 1) / a.jpiece;
    a.times_out = d_times;
    a.jumps_out = d_jumps;
    a.branch_out = d_branch;
    PML_TRY(mem.get(&a.partial, (size_t)cols * a.n_pieces * 2 * k));
    PML_TRY(mem.get(&a.xa, (size_t)cols * k));
    if (d_jumps != nullptr) {
        PML_TRY(mem.get(&a.stage, (size_t)cols * N * 3));
        PML_TRY(mem.get(&a.jpartial, (size_t)cols * a.n_jpieces * k * k));
    }
    with_branch_shape(k, [&](auto G, auto R) {
        hipLaunchKernelGGL((history_branch_kernel<G(), R()>), dim3(a.n_pieces, cols), dim3(256), 0, ctx->stream, a);
    });
    hipLaunchKernelGGL(history_vector_kernel, dim3(cols), dim3(256), 0, ctx->stream, a);
    if (d_jumps != nullptr) {
        const int T = (k + 15) / 16, TG = (T + 3) / 4;
        if (TG == 1) hipLaunchKernelGGL(history_jump_kernel<0>, dim3(a.n_jpieces, 1, cols), dim3(256), 0, ctx->stream, a);
        else hipLaunchKernelGGL(history_jump_kernel<1>, dim3(a.n_jpieces, TG * TG, cols), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(history_matrix_kernel, dim3((k * k + 255) / 256, cols), dim3(256), 0, ctx->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
