// Launches of the exact gradient of ln L of the F81 family (pml_kernels_gradient.h): the branch pass and the sum of the
// partials, for the columns [cb, ce) of the context in one go, queued on the context's stream.  pml_loglik_gradient (pml_api_readers.hip) checks the arguments, makes
// sure every vector the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_gradient.h"

// Ids per piece: fixed by k, never by the grid (the sums' order, hence their bits, follows from it).  A piece's partial is
// k + 3 doubles against the 2 k doubles each of its branches streams in: under 1 % of the traffic everywhere.  The sizes follow
// the lane shapes -- 256, 64 or 16, and 4 branches in flight per workgroup -- so that a workgroup makes 4 to 64 steps and a
// single column of a few thousand nodes still spreads over several workgroups.
static int gradient_piece(int k) { return k <= 4 ? 1024 : (k <= 64 ? 512 : 256); }

// d_rates [cols][3], d_pi [cols][k], d_flat [cols]; the partials live in the caller's scope, which makes the call's one wait
PML_INTERNAL int launch_gradient(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_rates, double* d_pi, int* d_flat) {
    const int k = ctx->k, N = ctx->N, cols = ce - cb;
    PmlGradArgs a;
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
    a.N = N;
    a.k = k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.col0 = cb;
    a.piece = gradient_piece(k);
    a.n_pieces = (N + a.piece - 1) / a.piece;
    a.rates_out = d_rates;
    a.pi_out = d_pi;
    a.flat_out = d_flat;
    PML_TRY(mem.get(&a.partial, (size_t)cols * a.n_pieces * (k + 3)));
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    with_branch_shape(k, [&](auto G, auto R) {
        hipLaunchKernelGGL((gradient_f81_kernel<G(), R()>), dim3(a.n_pieces, cols), dim3(256), 0, ctx->stream, a);
    });
    hipLaunchKernelGGL(gradient_reduce_kernel, dim3(cols), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
