// Launches of the history sampler of the F81 family (pml_kernels_history_sample.h) for one column: the walk over (piece, tile of
// repetitions) items and the sum of the pieces' partials, queued on the context's stream behind launch_scenarios, whose states
// it reads from the device.  pml_sample_histories (pml_api_readers.hip) checks the arguments, makes sure every vector the kernels read
// is in HBM, zeroes the counters and copies out.
#include "pml_launch.h"
#include "pml_kernels_history_sample.h"

// Ids per piece: 64 ceil(max(64, ceil(N / 256)) / 64) -- fixed by N, never by the grid or by k (the sums' order, hence their
// bits, follows from it): at most 256 pieces, so that the partials stay 256 rows per repetition at most, and at least 64 ids,
// so that a workgroup's table and its transposed write are spread over enough branches.
static int hsamp_piece(int N) { return 64 * ((std::max(64, (N + 255) / 256) + 63) / 64); }

#define PML_HSAMP_LDS_BYTES (136 * 1024)   // of the 160 KiB of a CU; 256 states at 64 repetitions take 134 KiB

// Repetitions per workgroup (one per thread).  The accumulators take k (T + 1) doubles of LDS, so the wavefronts a CU holds do
// not depend on T (about 160 KiB / (512 k) bytes); T only sets how many workgroups share the (piece, repetitions) items.  The
// largest of 256, 128 and 64 that fits: measured at 65 536 tips x 1024 repetitions (profiles/history_sampler.txt), 256 against
// 64 is 4 % less time at k = 4 and 5 % less at k = 64 (one workgroup of four wavefronts per CU instead of four of one).
static int hsamp_tile(int k, int n_rep) {
    int T = 64;
    for (int t : {128, 256})
        if (((size_t)k * (t + 1) + 2 * (size_t)k) * sizeof(double) <= PML_HSAMP_LDS_BYTES) T = t;
    return std::min(T, 64 * ((n_rep + 63) / 64));
}

PML_INTERNAL int launch_history_sample(pml_ctx* ctx, CallScope& mem, int col, int n_rep, int rep_offset, u64 seed, const void* d_states,
                                       size_t rs, double* d_times, unsigned* d_jumps, unsigned short* d_branch,
                                       unsigned long long* d_skipped) {
    const int k = ctx->k, N = ctx->N;
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    const bool wide = k > PML_HSAMP_LDS_K;
    PmlHsampArgs a;
    a.parent = ctx->d_parent;
    a.new_of_old = ctx->d_new_of_old;   // (both null when the library works in the caller's numbering)
    a.old_of_new = ctx->d_old_of_new;
    a.dist = ctx->d_dist;
    a.pi = ctx->d_pi + (size_t)col * ctx->ks;
    a.E = ctx->d_E + (size_t)col * N;
    a.mu = ctx->d_mu + col;
    a.sf = ctx->d_sf + col;
    a.tau = ctx->d_tau + col;
    a.tauf = ctx->d_tauf + col;
    a.N = N;
    a.k = k;
    a.piece = hsamp_piece(N);
    a.n_pieces = (N + a.piece - 1) / a.piece;
    const int T = wide ? 64 : hsamp_tile(k, n_rep);
    a.n_tiles = (n_rep + T - 1) / T;
    a.n_rep = n_rep;
    a.rs = rs;
    a.states = d_states;
    a.rep_offset = (unsigned)rep_offset;
    a.seed = seed;
    a.times_out = d_times;
    a.jumps = d_jumps;
    a.branch = d_branch;
    a.n_skipped = d_skipped;
    const size_t n_partial = (size_t)a.n_pieces * n_rep * k;
    PML_TRY(mem.get(&a.partial, n_partial));
    const long long items = (long long)a.n_pieces * a.n_tiles;
    if (items > 0x7fffffffll) return fail(PML_ERR_INVALID, "pml_sample_histories: %lld work items; draw fewer repetitions per call", items);
    if (wide) {
        // the accumulators are the partials themselves
        HIP_TRY(hipMemsetAsync(a.partial, 0, n_partial * sizeof(double), ctx->stream));
        hipLaunchKernelGGL(hsamp_kernel<true>, dim3((unsigned)items), dim3(T), (size_t)2 * k * sizeof(double), ctx->stream, a);
    } else {
        const size_t lds = ((size_t)k * (T + 1) + 2 * (size_t)k) * sizeof(double);   // (at most PML_HSAMP_LDS_BYTES)
        if (lds > 64 * 1024) PML_TRY(with_lds(ctx, hsamp_kernel<false>, lds));
        hipLaunchKernelGGL(hsamp_kernel<false>, dim3((unsigned)items), dim3(T), lds, ctx->stream, a);
    }
    HIP_TRY(hipGetLastError());
    const size_t total = (size_t)n_rep * k;
    hipLaunchKernelGGL(hsamp_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
