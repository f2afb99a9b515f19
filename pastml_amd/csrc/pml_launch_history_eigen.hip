// Launches of the exact expected dwell times and Markov jumps of the eigen-decomposed models (pml_kernels_history_eigen.h): the
// changes of basis, the pair sum, the sums of the partials and the final transforms, for the columns [cb, ce) of the context in
// one go, queued on the context's stream.  pml_expected_history_eigen (pml_api_readers.hip) checks the arguments, makes sure every vector
// the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_history_eigen.h"

// values of c a lane of the pair sum keeps in registers: the smallest band that covers k up to 32; two bands of 32 up to 64 states
// (168 registers and three wavefronts per SIMD where one band of 64 takes 256 and runs alone); beyond, bands of 64, which halve
// the number of tiles that read a branch's staged vectors again.  A pair's sum does not depend on the band it falls into.
int heig_rows(int k) { return k <= 4 ? 4 : (k <= 16 ? 16 : (k <= 64 ? 32 : 64)); }

void heig_args(const pml_ctx* ctx, int cb, PmlHeigArgs& a) {
    a = PmlHeigArgs{};   // (the pieces, the scratch and the outputs: the caller's)
    a.parent = ctx->d_parent;
    a.n_children = ctx->d_n_children;
    a.new_of_old = ctx->d_new_of_old;   // (null when the library works in the caller's numbering)
    a.dist = ctx->d_dist;
    a.masks = ctx->d_masks;
    a.bu = ctx->d_bu;
    a.post = ctx->d_post;
    a.ev = ctx->d_d;
    a.A = ctx->d_A;
    a.Ainv = ctx->d_Ainv;
    a.sf = ctx->d_sf;
    a.tau = ctx->d_tau;
    a.tauf = ctx->d_tauf;
    a.N = ctx->N;
    a.k = ctx->k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.col0 = cb;
    const int CR = heig_rows(ctx->k);
    a.tc = (ctx->k + CR - 1) / CR;
    a.td = (ctx->k + 63) / 64;
}

void launch_heig_basis(pml_ctx* ctx, int cols, const PmlHeigArgs& a) {
    const int kp = (a.k + 15) & ~15;
    const size_t lds = (size_t)(16 * (kp + 1) + 16) * sizeof(double);   // (35 KB at 256 states)
    const dim3 tiles((a.N + 15) / 16, cols);
    if (a.k >= 16) hipLaunchKernelGGL(heig_basis_kernel<true>, tiles, dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(heig_basis_kernel<false>, tiles, dim3(256), lds, ctx->stream, a);
}

// d_times [cols][k]; d_jumps [cols][k][k] or null; d_branch [cols][N] (caller's numbering) or null.  Queued only: the staged
// vectors and the partials live in the caller's scope, which makes the call's one wait.
PML_INTERNAL int launch_history_eigen(pml_ctx* ctx, CallScope& mem, int cb, int ce, double* d_times, double* d_jumps, double* d_branch) {
    const int k = ctx->k, N = ctx->N, cols = ce - cb;
    if (k < 2 || k > 256) return fail(PML_ERR_UNSUPPORTED, "k = %d: the eigen models' history takes 2 to 256 states", k);
    PmlHeigArgs a;
    heig_args(ctx, cb, a);
    a.n_pieces = (N + PML_HEIG_PIECE - 1) / PML_HEIG_PIECE;
    a.times_out = d_times;
    a.jumps_out = d_jumps;
    a.branch_out = d_branch;
    const size_t kk = (size_t)k * k;
    PML_TRY(mem.get(&a.stage, (size_t)cols * N * 3 * ctx->ks));
    PML_TRY(mem.get(&a.tprime, (size_t)cols * N));
    PML_TRY(mem.get(&a.partial, (size_t)cols * a.n_pieces * kk));
    PML_TRY(mem.get(&a.Wsum, (size_t)cols * kk));
    PML_TRY(mem.get(&a.T1, (size_t)cols * kk));
    const dim3 square((unsigned)((kk + 255) / 256), cols);
    if (d_branch != nullptr) {
        PML_TRY(mem.get(&a.qdiag, (size_t)cols * k));
        PML_TRY(mem.get(&a.G, (size_t)cols * kk));
        PML_TRY(mem.get(&a.bpart, (size_t)cols * a.tc * a.td * N));
        hipLaunchKernelGGL(heig_qdiag_kernel, dim3(cols), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(heig_g_kernel, square, dim3(256), 0, ctx->stream, a);
    }
    launch_heig_basis(ctx, cols, a);
    with_heig_rows(k, [&](auto CR) {
        hipLaunchKernelGGL(heig_pair_kernel<CR()>, dim3(a.n_pieces, a.tc * a.td, cols), dim3(256), 0, ctx->stream, a);
    });
    hipLaunchKernelGGL(heig_reduce_kernel, square, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(heig_t1_kernel, square, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(heig_times_kernel, dim3(cols), dim3(256), 0, ctx->stream, a);
    if (d_jumps != nullptr) hipLaunchKernelGGL(heig_jumps_kernel, square, dim3(256), 0, ctx->stream, a);
    if (d_branch != nullptr) hipLaunchKernelGGL(heig_branch_kernel, dim3((N + 255) / 256, cols), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
