// Launches of the forward simulator (pml_kernels_simulate.h): the schedule over the depth levels and the subtrees below a
// frontier depth.  pml_simulate_states (pml_api_readers.hip) checks the arguments, runs the per-branch preparation and copies out.
#include "pml_launch.h"
#include "pml_kernels_simulate.h"

// Schedule.  The top depth levels are one launch each (a list per node); the subtrees rooted at the frontier depth D are one
// launch in which a workgroup walks a subtree in preorder for its repetition tile -- no grid-wide dependency, so a deep tree
// (a 10^4-deep caterpillar) costs D + 1 launches, not one per level.  D is the first depth whose nodes times the repetition
// tiles give PML_SIM_ITEMS workgroups, and at most PML_SIM_MAX_TOP.
#define PML_SIM_ITEMS 2048
#define PML_SIM_MAX_TOP 16
#define PML_SIM_SCRATCH_BYTES (256ull << 20)   // bound of the cumulative rows of wide matrix models (PML_SIM_MATRIX_SCRATCH)

PML_INTERNAL int sim_frontier_depth(const pml_ctx* ctx, int n_tiles) {
    const int L = ctx->n_td_levels;
    for (int d = 0; d < L; ++d) {
        const long long cnt = ctx->forest.td_offsets[d + 1] - ctx->forest.td_offsets[d];
        if (cnt * n_tiles >= PML_SIM_ITEMS || d >= PML_SIM_MAX_TOP) return d;
    }
    return L;   // (a shallow forest: level launches only)
}

// preorder lists of the subtrees rooted at depth D (entries: PmlSimArgs::lists), uploaded once per (tree, D)
PML_INTERNAL int sim_subtree_lists(pml_ctx* ctx, int D) {
    if (ctx->sim_depth == D) return PML_OK;
    const int r0 = ctx->forest.td_offsets[D], r1 = ctx->forest.td_offsets[D + 1];
    const int* fc = ctx->forest.first_child.data();   // (the library's numbering: a node's children are fc[n] .. fc[n] + nc - 1)
    const bool perm = !ctx->old_of_new.empty();
    auto api = [&](int n) { return perm ? ctx->old_of_new[n] : n; };   // the caller's id of an internal node
    std::vector<int4> lists;
    std::vector<int> off(1, 0), stack;
    lists.reserve((size_t)(ctx->N - r0));
    for (int r = r0; r < r1; ++r) {
        stack.assign(1, r);
        while (!stack.empty()) {
            const int n = stack.back();
            stack.pop_back();
            const int p = ctx->forest.parent[n];
            lists.push_back(make_int4(n, api(n), p < 0 ? -1 : api(p), 0));
            for (int j = ctx->forest.n_children[n] - 1; j >= 0; --j) stack.push_back(fc[n] + j);
        }
        off.push_back((int)lists.size());
    }
    if (ctx->d_sim_lists) (void)hipFree(ctx->d_sim_lists);
    if (ctx->d_sim_off) (void)hipFree(ctx->d_sim_off);
    ctx->d_sim_lists = nullptr;
    ctx->d_sim_off = nullptr;
    ctx->sim_depth = -1;
    HIP_TRY(hipMalloc((void**)&ctx->d_sim_lists, std::max<size_t>(1, lists.size()) * sizeof(int4)));
    HIP_TRY(hipMalloc((void**)&ctx->d_sim_off, off.size() * sizeof(int)));
    HIP_TRY(hipMemcpyAsync(ctx->d_sim_lists, lists.data(), lists.size() * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->d_sim_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));   // (the host vectors go out of scope)
    ctx->sim_n_lists = r1 - r0;
    ctx->sim_depth = D;
    return PML_OK;
}

// The windowed form of the schedule (pml_pij_window.h: pml_plan_sim_window), uploaded for one call: the branch lists of the runs
// and the preorder lists of the frontier subtrees, whose entries carry their slot in the group's window.  The context's own
// lists (sim_subtree_lists) are left alone: the frontier of a windowed call may lie deeper.
PML_INTERNAL int sim_window_prepare(pml_ctx* ctx, int D, CallScope& mem, SimWindowDevice& w) {
    const std::string bad = pml_plan_sim_window(ctx->forest, D, ctx->pij_window, w.plan);
    if (!bad.empty()) return fail(PML_ERR_INVALID, "%s", bad.c_str());
    const bool perm = !ctx->old_of_new.empty();
    auto api = [&](int n) { return perm ? ctx->old_of_new[n] : n; };
    const PmlSimWindowPlan& P = w.plan;
    w.lists.resize(P.order.size() - (size_t)P.list_base);
    for (const PmlSimWindowRun& g : P.groups)
        for (int i = 0; i < g.build_count; ++i) {
            const int n = P.order[(size_t)(g.build_first + i)];
            const int p = ctx->forest.parent[n];
            w.lists[(size_t)(g.build_first - P.list_base + i)] = make_int4(n, api(n), p < 0 ? -1 : api(p), i);
        }
    PML_TRY(mem.put(&w.d_order, (const int*)P.order.data(), P.order.size()));
    PML_TRY(mem.put(&w.d_lists, (const int4*)w.lists.data(), w.lists.size()));
    PML_TRY(mem.put(&w.d_off, (const int*)P.sub_off.data(), P.sub_off.size()));
    return PML_OK;
}

template <typename T, int MODE, bool WIN = false>
static int sim_launch(pml_ctx* ctx, PmlSimArgs a, int threads, size_t lds, long long max_blocks) {
    const long long items = (long long)a.n_lists * a.n_tiles;
    if (items <= 0) return PML_OK;
    const int blocks = (int)std::min<long long>(items, max_blocks);
    if (lds > 64 * 1024) PML_TRY(with_lds(ctx, simulate_kernel<T, MODE, WIN>, lds));
    hipLaunchKernelGGL((simulate_kernel<T, MODE, WIN>), dim3(blocks), dim3(threads), lds, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}

template <typename T, int MODE>
static int sim_run(pml_ctx* ctx, PmlSimArgs a, int threads, int D, size_t lds, long long max_blocks) {
    for (int d = 0; d < D; ++d) {
        a.lists = nullptr;
        a.list_off = nullptr;
        a.first_node = ctx->forest.td_offsets[d];
        a.n_lists = ctx->forest.td_offsets[d + 1] - ctx->forest.td_offsets[d];
        PML_TRY((sim_launch<T, MODE>(ctx, a, threads, lds, max_blocks)));
    }
    if (D < ctx->n_td_levels) {
        a.lists = ctx->d_sim_lists;
        a.list_off = ctx->d_sim_off;
        a.first_node = 0;
        a.n_lists = ctx->sim_n_lists;
        PML_TRY((sim_launch<T, MODE>(ctx, a, threads, lds, max_blocks)));
    }
    return PML_OK;
}

PML_INTERNAL int launch_simulate(pml_ctx* ctx, int col, int rep_offset, u64 seed, void* d_states, size_t rs) {
    const int k = ctx->k;
    const int n_tuples = (int)(rs / 4);
    const int threads = std::min(PML_SIM_THREADS, 64 * ((n_tuples + 63) / 64));
    const int n_tiles = (n_tuples + threads - 1) / threads;
    const int D = sim_frontier_depth(ctx, n_tiles);
    const bool windowed = pij_windowed(ctx);
    if (D < ctx->n_td_levels && !windowed) PML_TRY(sim_subtree_lists(ctx, D));
    PmlSimArgs a;
    a.parent = ctx->d_parent;
    a.api_id = ctx->d_old_of_new;   // (null when the library works in the caller's numbering)
    a.lists = nullptr;
    a.list_off = nullptr;
    a.first_node = 0;
    a.n_lists = 0;
    a.n_tiles = n_tiles;
    a.n_tuples = n_tuples;
    a.rs = rs;
    a.states = d_states;
    a.rep_offset = (unsigned)rep_offset;
    a.seed = seed;
    a.k = k;
    a.ks = ctx->ks;
    a.pi = ctx->d_pi + (size_t)col * ctx->ks;
    a.E = ctx->kind == PML_MODEL_F81 ? ctx->d_E + (size_t)col * ctx->N : nullptr;
    a.P = ctx->kind == PML_MODEL_F81 ? nullptr : ctx->d_P + (size_t)col * ctx->N * k * ctx->ks;
    a.scratch = nullptr;
    const long long cap = 1 << 20;
    if (windowed) {
        // P(t) from the context's window, built run by run for this column (its window is the first of the buffer)
        SimWindowDevice w;
        CallScope mem(ctx->stream, false);
        PML_TRY(sim_window_prepare(ctx, D, mem, w));
        a.P = ctx->d_pij_window;
        if (k <= PML_SIM_LDS_K) {
            const size_t lds = (size_t)(k + k * k) * sizeof(double);
            PML_TRY(sim_window_run(ctx, a, w, col, [&](const PmlSimArgs& x) {
                return sim_launch<unsigned char, PML_SIM_MATRIX_LDS, true>(ctx, x, threads, lds, cap);
            }));
        } else {
            const long long blocks = std::max<long long>(1, (long long)(PML_SIM_SCRATCH_BYTES / ((size_t)k * k * sizeof(double))));
            PML_TRY(mem.get(&a.scratch, (size_t)blocks * k * k));
            PML_TRY(sim_window_run(ctx, a, w, col, [&](const PmlSimArgs& x) {
                return sim_launch<unsigned char, PML_SIM_MATRIX_SCRATCH, true>(ctx, x, threads, (size_t)k * sizeof(double), blocks);
            }));
        }
        return mem.finish();
    }
    if (ctx->kind == PML_MODEL_F81) {
        const size_t lds = (size_t)k * sizeof(double);
        if (k > 256) return sim_run<unsigned short, PML_SIM_F81>(ctx, a, threads, D, lds, cap);
        return sim_run<unsigned char, PML_SIM_F81>(ctx, a, threads, D, lds, cap);
    }
    if (k <= PML_SIM_LDS_K)
        return sim_run<unsigned char, PML_SIM_MATRIX_LDS>(ctx, a, threads, D, (size_t)(k + k * k) * sizeof(double), cap);
    // wide matrix models: a slice of k x k doubles per workgroup, the grid bounded by PML_SIM_SCRATCH_BYTES
    const size_t slice = (size_t)k * k * sizeof(double);
    const long long blocks = std::max<long long>(1, (long long)(PML_SIM_SCRATCH_BYTES / slice));
    CallScope mem(ctx->stream, false);
    PML_TRY(mem.get(&a.scratch, (size_t)blocks * k * k));
    PML_TRY((sim_run<unsigned char, PML_SIM_MATRIX_SCRATCH>(ctx, a, threads, D, (size_t)k * sizeof(double), blocks)));
    return mem.finish();   // (the scratch goes)
}
