// Launches of the scenario sampler (pml_kernels_scenarios.h) over the forward simulator's schedule: the top depth levels one
// launch each, the subtrees below the frontier depth in one launch (pml_launch_simulate.hip).  pml_sample_scenarios
// (pml_api_readers.hip) checks the arguments, makes sure every vector the kernel reads is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_scenarios.h"

#define PML_SCEN_SCRATCH_BYTES (256ull << 20)   // bound of the cumulative rows of wide matrix models (PML_SIM_MATRIX_SCRATCH)

template <typename T, int MODE, bool WIN = false>
static int scen_launch(pml_ctx* ctx, PmlScenArgs a, int threads, size_t lds, long long max_blocks) {
    const long long items = (long long)a.n_lists * a.n_tiles;
    if (items <= 0) return PML_OK;
    const int blocks = (int)std::min<long long>(items, max_blocks);
    if (lds > 64 * 1024) PML_TRY(with_lds(ctx, scenarios_kernel<T, MODE, WIN>, lds));
    hipLaunchKernelGGL((scenarios_kernel<T, MODE, WIN>), dim3(blocks), dim3(threads), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}

template <typename T, int MODE>
static int scen_run(pml_ctx* ctx, PmlScenArgs a, int threads, int D, size_t lds, long long max_blocks) {
    for (int d = 0; d < D; ++d) {
        a.lists = nullptr;
        a.list_off = nullptr;
        a.first_node = ctx->forest.td_offsets[d];
        a.n_lists = ctx->forest.td_offsets[d + 1] - ctx->forest.td_offsets[d];
        PML_TRY((scen_launch<T, MODE>(ctx, a, threads, lds, max_blocks)));
    }
    if (D < ctx->n_td_levels) {
        a.lists = ctx->d_sim_lists;
        a.list_off = ctx->d_sim_off;
        a.first_node = 0;
        a.n_lists = ctx->sim_n_lists;
        PML_TRY((scen_launch<T, MODE>(ctx, a, threads, lds, max_blocks)));
    }
    return PML_OK;
}

PML_INTERNAL int launch_scenarios(pml_ctx* ctx, int col, int n_rep, int rep_offset, u64 seed, void* d_states, size_t rs,
                                  unsigned long long* d_fallback) {
    const int k = ctx->k;
    const bool f81 = ctx->kind == PML_MODEL_F81;
    if (k > (f81 ? 512 : 256))
        return fail(PML_ERR_UNSUPPORTED, "k = %d: the scenario sampler holds at most %d states for this model", k, f81 ? 512 : 256);
    const int n_tuples = (int)(rs / 4);
    const int threads = std::min(PML_SIM_THREADS, 64 * ((n_tuples + 63) / 64));
    const int n_tiles = (n_tuples + threads - 1) / threads;
    const int D = sim_frontier_depth(ctx, n_tiles);
    const bool windowed = pij_windowed(ctx);
    if (D < ctx->n_td_levels && !windowed) PML_TRY(sim_subtree_lists(ctx, D));
    const size_t colN = (size_t)col * ctx->N;
    PmlScenArgs a;
    a.parent = ctx->d_parent;
    a.api_id = ctx->d_old_of_new;   // (null when the library works in the caller's numbering)
    a.n_children = ctx->d_n_children;
    a.lists = nullptr;
    a.list_off = nullptr;
    a.first_node = 0;
    a.n_lists = 0;
    a.n_tiles = n_tiles;
    a.n_tuples = n_tuples;
    a.n_rep = n_rep;
    a.rs = rs;
    a.states = d_states;
    a.rep_offset = (unsigned)rep_offset;
    a.seed = seed;
    a.k = k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.pi = ctx->d_pi + (size_t)col * ctx->ks;
    a.masks = ctx->d_masks + colN * ctx->W;
    a.bu = ctx->d_bu + colN * ctx->ks;
    a.post = ctx->d_post + colN * ctx->ks;
    a.E = f81 ? ctx->d_E + colN : nullptr;
    a.P = f81 ? nullptr : ctx->d_P + colN * k * ctx->ks;
    a.scratch = nullptr;
    a.n_fallback = d_fallback;
    const long long cap = 1 << 20;
    if (windowed) {
        // P(t) from the context's window, built run by run for this column (its window is the first of the buffer)
        SimWindowDevice w;
        CallScope mem(ctx->stream, false);
        PML_TRY(sim_window_prepare(ctx, D, mem, w));
        a.P = ctx->d_pij_window;
        if (k <= PML_SIM_LDS_K) {
            const size_t lds = (size_t)(k + k * k) * sizeof(double);
            PML_TRY(sim_window_run(ctx, a, w, col, [&](const PmlScenArgs& x) {
                return scen_launch<unsigned char, PML_SIM_MATRIX_LDS, true>(ctx, x, threads, lds, cap);
            }));
        } else {
            const long long blocks = std::max<long long>(1, (long long)(PML_SCEN_SCRATCH_BYTES / ((size_t)k * k * sizeof(double))));
            PML_TRY(mem.get(&a.scratch, (size_t)blocks * k * k));
            PML_TRY(sim_window_run(ctx, a, w, col, [&](const PmlScenArgs& x) {
                return scen_launch<unsigned char, PML_SIM_MATRIX_SCRATCH, true>(ctx, x, threads, (size_t)k * sizeof(double), blocks);
            }));
        }
        return mem.finish();
    }
    if (f81) {
        const size_t lds = (size_t)3 * k * sizeof(double);
        if (k > 256) return scen_run<unsigned short, PML_SIM_F81>(ctx, a, threads, D, lds, cap);
        return scen_run<unsigned char, PML_SIM_F81>(ctx, a, threads, D, lds, cap);
    }
    if (k <= PML_SIM_LDS_K)
        return scen_run<unsigned char, PML_SIM_MATRIX_LDS>(ctx, a, threads, D, (size_t)(k + k * k) * sizeof(double), cap);
    // wide matrix models: a slice of k x k doubles per workgroup, the grid bounded by PML_SCEN_SCRATCH_BYTES
    const size_t slice = (size_t)k * k * sizeof(double);
    const long long blocks = std::max<long long>(1, (long long)(PML_SCEN_SCRATCH_BYTES / slice));
    CallScope mem(ctx->stream, false);
    PML_TRY(mem.get(&a.scratch, (size_t)blocks * k * k));
    PML_TRY((scen_run<unsigned char, PML_SIM_MATRIX_SCRATCH>(ctx, a, threads, D, (size_t)k * sizeof(double), blocks)));
    return mem.finish();   // (the scratch goes)
}
