// Launches of the vertical collapse (pml_kernels_compress.h): scratch, chunking over the columns, the rounds of the pointer
// jumping.  pml_compress_vertical (pml_api.hip) checks the arguments.
#include "pml_launch.h"
#include "pml_kernels_compress.h"

namespace {

struct Scratch {
    std::vector<void*> p;
    ~Scratch() {
        for (void* q : p) (void)hipFree(q);
    }
    template <typename T>
    int get(T** out, size_t count) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(1, count) * sizeof(T));
        if (e != hipSuccess) return fail(PML_ERR_HIP, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        p.push_back(q);
        *out = (T*)q;
        return PML_OK;
    }
};

// the brackets of the passes for pml_compress_vertical_info: events only while the context profiles (pml_profile_enable)
struct Events {
    bool on;
    std::vector<hipEvent_t> ev;
    explicit Events(bool on_) : on(on_) {}
    ~Events() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int mark(hipStream_t s) {
        if (!on) return PML_OK;
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
        HIP_TRY(hipEventRecord(e, s));
        return PML_OK;
    }
};

}  // namespace

PML_INTERNAL int launch_compress(pml_ctx* ctx, int n_cols, int W, const u64* sets, const unsigned char* is_polytomy, int* top_out,
                                 int* tips_out, int* internal_out, int* parent_vertex_out) {
    const int N = ctx->N;
    int WG = 1;
    while (WG < W) WG <<= 1;
    const size_t col_words = (size_t)N * W;
    // the deepest node is n_td_levels - 1 branches below its root: after r rounds every node has looked 2^r nodes up
    const int deepest = std::max(0, ctx->n_td_levels - 1);
    int rounds = 0;
    while ((1ll << rounds) < deepest) ++rounds;

    // columns per chunk: what the scratch allows (half of the free memory at most)
    HIP_TRY(hipSetDevice(ctx->device));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t per_col = col_words * 8;
    long long chunk = (long long)std::min<size_t>(free_b / 2 / std::max<size_t>(1, per_col), 1 << 20);
    if (ctx->tune.on(T_COMPRESS_MAX_COLS)) chunk = std::min(chunk, std::max(1ll, ctx->tune.get(T_COMPRESS_MAX_COLS, 1)));
    if (chunk < 1) return fail(PML_ERR_HIP, "pml_compress_vertical: %zu bytes of scratch per column do not fit the device", per_col);
    chunk = std::min<long long>(chunk, n_cols);

    Scratch mem;
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
    if (is_polytomy) PML_TRY(mem.get(&d_pol, (size_t)N));

    hipStream_t s = ctx->stream;
    const bool perm = !ctx->old_of_new.empty();
    const int node_blocks = (N + PML_COMPRESS_THREADS - 1) / PML_COMPRESS_THREADS;
    const int per_block = PML_COMPRESS_THREADS / WG;
    const int differs_blocks = (int)std::min<long long>(((long long)N + per_block - 1) / per_block, 1 << 20);
    Events ev(ctx->profile);
    double merged_ms = 0;

    if (is_polytomy) HIP_TRY(hipMemcpyAsync(d_pol, is_polytomy, (size_t)N, hipMemcpyHostToDevice, s));
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
        PML_TRY(ev.mark(s));
        hipLaunchKernelGGL(compress_differs_kernel, dim3(differs_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_sets, d_parent, d_differs,
                           N, W, WG, cc);
        HIP_TRY(hipGetLastError());
        PML_TRY(ev.mark(s));
    }
    const size_t after_merged = ev.ev.size();
    PML_TRY(ev.mark(s));
    hipLaunchKernelGGL(compress_top_init_kernel, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_parent, d_differs, d_top, N);
    HIP_TRY(hipGetLastError());
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(compress_jump_kernel, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, N);
        HIP_TRY(hipGetLastError());
    }
    PML_TRY(ev.mark(s));
    if (ctx->tune.on(T_COMPRESS_PLAIN_ATOMICS))
        hipLaunchKernelGGL(compress_counts_kernel<false>, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, d_parent, d_kind,
                           d_tips, d_internal, d_pv, N);
    else
        hipLaunchKernelGGL(compress_counts_kernel<true>, dim3(node_blocks), dim3(PML_COMPRESS_THREADS), 0, s, d_top, d_parent, d_kind,
                           d_tips, d_internal, d_pv, N);
    HIP_TRY(hipGetLastError());
    PML_TRY(ev.mark(s));
    HIP_TRY(hipMemcpyAsync(top_out, d_top, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tips_out, d_tips, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(internal_out, d_internal, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(parent_vertex_out, d_pv, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float jump_ms = 0.f, counts_ms = 0.f;
    if (ev.on) {
        for (size_t i = 0; i + 1 < after_merged; i += 2) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, ev.ev[i], ev.ev[i + 1]));
            merged_ms += ms;
        }
        HIP_TRY(hipEventElapsedTime(&jump_ms, ev.ev[after_merged], ev.ev[after_merged + 1]));
        HIP_TRY(hipEventElapsedTime(&counts_ms, ev.ev[after_merged + 1], ev.ev[after_merged + 2]));
    }
    ctx->compress_ms[0] = merged_ms;
    ctx->compress_ms[1] = jump_ms;
    ctx->compress_ms[2] = counts_ms;
    ctx->compress_rounds = rounds;
    return PML_OK;
}
