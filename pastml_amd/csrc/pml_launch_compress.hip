// Launches of the vertical collapse (pml_kernels_compress.h): the chunks of columns, the rounds of the pointer jumping; the
// scratch and the event brackets live in a CallScope (pml_call_scope.h).  pml_compress_vertical (pml_api.hip) checks the arguments.
#include "pml_launch.h"
#include "pml_kernels_compress.h"

PML_INTERNAL int launch_compress(pml_ctx* ctx, int n_cols, int W, const u64* sets, const unsigned char* is_polytomy, int* top_out,
                                 int* tips_out, int* internal_out, int* parent_vertex_out) {
    const int N = ctx->N;
    const int WG = (int)pow2_from((size_t)W);
    const size_t col_words = (size_t)N * W;
    // the deepest node is n_td_levels - 1 branches below its root: after r rounds every node has looked 2^r nodes up
    const int deepest = std::max(0, ctx->n_td_levels - 1);
    int rounds = 0;
    while ((1ll << rounds) < deepest) ++rounds;

    // columns per chunk: what the scratch allows (half of the free memory at most)
    long long chunk;
    PML_TRY(columns_per_chunk(ctx, col_words * 8, 1 << 20, T_COMPRESS_MAX_COLS, n_cols, "pml_compress_vertical", &chunk));

    hipStream_t s = ctx->stream;
    CallScope mem(s, ctx->profile);   // (events for pml_compress_vertical_info only while the context profiles)
    u64* d_sets;
    int *d_parent, *d_top, *d_tips, *d_internal, *d_pv;
    unsigned char *d_kind, *d_differs, *d_pol = nullptr;
    PML_TRY(mem.get(&d_sets, (size_t)chunk * col_words));
    PML_TRY(mem.get(&d_parent, (size_t)N));
    PML_TRY(mem.get(&d_top, (size_t)N));
    PML_TRY(mem.get(&d_tips, (size_t)N));
    PML_TRY(mem.get(&d_internal, (size_t)N));
    PML_TRY(mem.get(&d_pv, (size_t)N));
    PML_TRY(mem.get(&d_kind, (size_t)N));
    PML_TRY(mem.get(&d_differs, (size_t)N));
    if (is_polytomy) PML_TRY(mem.put(&d_pol, is_polytomy, (size_t)N));

    const bool perm = !ctx->old_of_new.empty();
    const int node_blocks = (N + PML_COMPRESS_THREADS - 1) / PML_COMPRESS_THREADS;
    const int per_block = PML_COMPRESS_THREADS / WG;
    const int differs_blocks = (int)std::min<long long>(((long long)N + per_block - 1) / per_block, 1 << 20);
    double merged_ms = 0;

    HIP_TRY(hipMemsetAsync(d_differs, 0, (size_t)N, s));
    HIP_TRY(hipMemsetAsync(d_tips, 0, (size_t)N * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_internal, 0, (size_t)N * sizeof(int), s));
    hipLaunchKernelGGL(compress_tree_kernel, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, ctx->d_parent, ctx->d_n_children,
                       perm ? ctx->d_new_of_old : nullptr, perm ? ctx->d_old_of_new : nullptr, d_pol, d_parent, d_kind, N);
    HIP_TRY(hipGetLastError());
    for (int c0 = 0; c0 < n_cols; c0 += (int)chunk) {
        const int cc = std::min<int>((int)chunk, n_cols - c0);
        // (the copy of a chunk waits for the pass over the one before it: one stream, one buffer)
        HIP_TRY(hipMemcpyAsync(d_sets, sets + (size_t)c0 * col_words, (size_t)cc * col_words * 8, hipMemcpyHostToDevice, s));
        PML_TRY(mem.mark());
        hipLaunchKernelGGL(compress_differs_kernel, dim3(differs_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_sets, d_parent, d_differs,
                           N, W, WG, cc);
        HIP_TRY(hipGetLastError());
        PML_TRY(mem.mark());
    }
    const size_t after_merged = mem.n_marks();
    PML_TRY(mem.mark());
    hipLaunchKernelGGL(compress_top_init_kernel, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_parent, d_differs, d_top, N);
    HIP_TRY(hipGetLastError());
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(compress_jump_kernel, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, N);
        HIP_TRY(hipGetLastError());
    }
    PML_TRY(mem.mark());
    if (ctx->tune.on(T_COMPRESS_PLAIN_ATOMICS))
        hipLaunchKernelGGL(compress_counts_kernel<false>, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, d_parent, d_kind,
                           d_tips, d_internal, d_pv, N);
    else
        hipLaunchKernelGGL(compress_counts_kernel<true>, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, d_parent, d_kind,
                           d_tips, d_internal, d_pv, N);
    HIP_TRY(hipGetLastError());
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(top_out, d_top, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tips_out, d_tips, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(internal_out, d_internal, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(parent_vertex_out, d_pv, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    PML_TRY(mem.finish());
    float jump_ms = 0.f, counts_ms = 0.f;
    for (size_t i = 0; i + 1 < after_merged; i += 2) {
        float ms = 0.f;
        PML_TRY(mem.elapsed(i, i + 1, &ms));
        merged_ms += ms;
    }
    PML_TRY(mem.elapsed(after_merged, after_merged + 1, &jump_ms));
    PML_TRY(mem.elapsed(after_merged + 1, after_merged + 2, &counts_ms));
    ctx->compress_ms[0] = merged_ms;
    ctx->compress_ms[1] = jump_ms;
    ctx->compress_ms[2] = counts_ms;
    ctx->compress_rounds = rounds;
    return PML_OK;
}
