// Launches of the timeline (pml_kernels_timeline.h): the checks of the arrays (host, linear -- every index a kernel follows is
// checked here), the plan of the level sweeps -- a wide level is a launch of its own, a run of consecutive levels of at most
// PML_TL_FUSE nodes each is one launch of one workgroup --, the stages with an event between them.  pml_timeline (pml_api.hip)
// checks the pointers.
#include <cmath>
#include "pml_launch.h"
#include "pml_kernels_timeline.h"

namespace {
struct LevelRun {
    int d0, d1;   // levels [d0, d1)
    bool fused;   // one workgroup walks them all; else d1 == d0 + 1 and the level is spread over workgroups
};

std::vector<LevelRun> plan_levels(const int* level, int n_levels) {
    std::vector<LevelRun> runs;
    for (int d = 0; d < n_levels;) {
        if (level[d + 1] - level[d] > PML_TL_FUSE) {
            runs.push_back({d, d + 1, false});
            ++d;
            continue;
        }
        int e = d + 1;
        while (e < n_levels && level[e + 1] - level[e] <= PML_TL_FUSE) ++e;
        runs.push_back({d, e, true});
        d = e;
    }
    return runs;
}

int check_arrays(const pml_timeline_in& in) {
    const int N = in.n_nodes, D = in.n_levels;
    if (in.level_offsets[0] != 0 || in.level_offsets[D] != N) return fail(PML_ERR_INVALID, "level_offsets must run from 0 to n_nodes");
    for (int d = 0; d < D; ++d) {
        const int a = in.level_offsets[d], b = in.level_offsets[d + 1];
        if (a < 0 || b <= a || b > N) return fail(PML_ERR_INVALID, "level %d is empty or out of range: [%d, %d)", d, a, b);
        for (int n = a; n < b; ++n) {
            const int p = in.parent[n];
            if (d == 0 ? p != -1 : (p < in.level_offsets[d - 1] || p >= a))
                return fail(PML_ERR_INVALID, "parent[%d] = %d does not lie in the level above level %d", n, p, d);
        }
    }
    if (in.dates_only) return PML_OK;
    const int C = in.n_configs, T = in.n_tips, L = in.n_vertices, M = in.n_milestones;
    for (int n = 0; n < N; ++n) {
        if (in.up[n] < -1 || in.up[n] >= n) return fail(PML_ERR_INVALID, "up[%d] = %d: an ancestor has a smaller id", n, in.up[n]);
        if (in.config[n] < -1 || in.config[n] >= C) return fail(PML_ERR_INVALID, "config[%d] = %d is none of the %d", n, in.config[n], C);
    }
    for (int c = 0; c < C; ++c) {
        if (in.top[c] < 0 || in.top[c] >= N) return fail(PML_ERR_INVALID, "top[%d] = %d is no node", c, in.top[c]);
        if (in.below_lo[c] < 0 || in.below_lo[c] > in.below_hi[c] || in.below_hi[c] > T)
            return fail(PML_ERR_INVALID, "the tips below configuration %d, [%d, %d), are no run of the %d tips", c, in.below_lo[c],
                        in.below_hi[c], T);
    }
    for (int r = 0; r < T; ++r)
        if (in.tip_order[r] < 0 || in.tip_order[r] >= N) return fail(PML_ERR_INVALID, "tip_order[%d] = %d is no node", r, in.tip_order[r]);
    if (in.member_offsets[0] != 0 || in.member_offsets[L] != C) return fail(PML_ERR_INVALID, "member_offsets must run from 0 to n_configs");
    for (int v = 0; v < L; ++v)
        if (in.member_offsets[v + 1] < in.member_offsets[v]) return fail(PML_ERR_INVALID, "member_offsets[%d] decreases", v + 1);
    for (int i = 0; i < M; ++i)
        if (std::isnan(in.milestones[i]) || (i && !(in.milestones[i - 1] < in.milestones[i])))
            return fail(PML_ERR_INVALID, "the milestones must ascend strictly (milestone %d)", i);
    return PML_OK;
}
}   // namespace

#define TL_LAUNCH(kernel, grid, block, ...)                                 \
    do {                                                                    \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, __VA_ARGS__); \
        HIP_TRY(hipGetLastError());                                         \
        ++launches;                                                         \
    } while (0)

PML_INTERNAL int launch_timeline(pml_ctx* ctx, const pml_timeline_in& in, const pml_timeline_out& out) {
    PML_TRY(check_arrays(in));
    const int N = in.n_nodes, D = in.n_levels, C = in.n_configs, T = in.n_tips, L = in.n_vertices, M = in.n_milestones;
    const int R = in.level_offsets[1];
    const std::vector<LevelRun> runs = plan_levels(in.level_offsets, D);
    for (int i = 0; i < 6; ++i) ctx->tl_ms[i] = 0;
    ctx->tl_levels = D;
    ctx->tl_launches = ctx->tl_date_launches = 0;

    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    CallScope mem(s, ctx->profile);
    long long launches = 0;
    const int blocks = (N + PML_TL_THREADS - 1) / PML_TL_THREADS;

    // ---- dates ----------------------------------------------------------------------------------------------------------
    int *d_level, *d_parent;
    double *d_dist, *d_given, *d_root, *d_date;
    PML_TRY(mem.put(&d_level, (const int*)in.level_offsets, (size_t)D + 1));
    PML_TRY(mem.put(&d_parent, (const int*)in.parent, (size_t)N));
    PML_TRY(mem.put(&d_dist, in.dist, (size_t)N));
    PML_TRY(mem.put(&d_given, in.given, (size_t)N));
    PML_TRY(mem.put(&d_root, in.root_dates, (size_t)R));
    PML_TRY(mem.get(&d_date, (size_t)N));
    PML_TRY(mem.mark());
    for (const LevelRun& r : runs) {
        if (r.fused) {
            TL_LAUNCH(tl_dates_fused_kernel, 1, PML_TL_THREADS, r.d0, r.d1, d_level, d_parent, d_dist, d_given, d_root, d_date);
        } else {
            const int a = in.level_offsets[r.d0], b = in.level_offsets[r.d1];
            TL_LAUNCH(tl_dates_level_kernel, (b - a + PML_TL_THREADS - 1) / PML_TL_THREADS, PML_TL_THREADS, a, b, d_parent, d_dist, d_given,
                      d_root, d_date);
        }
    }
    ctx->tl_date_launches = launches;
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(out.date, d_date, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
    float ms = 0.f;
    if (in.dates_only) {
        PML_TRY(mem.finish());
        PML_TRY(mem.elapsed(0, 1, &ms));
        ctx->tl_ms[0] = ms;
        ctx->tl_launches = launches;
        return PML_OK;
    }

    // ---- get_date -------------------------------------------------------------------------------------------------------
    unsigned char *d_alive, *d_is_tip, *d_poly, *d_tbin;
    int *d_up, *d_config, *d_top, *d_lo, *d_hi, *d_order, *d_members, *d_bin, *d_cbin, *d_tips, *d_internal, *d_hist, *d_below;
    double *d_get, *d_miles;
    tl_u64 *d_smin = nullptr, *d_max = nullptr;
    PML_TRY(mem.put(&d_alive, (const unsigned char*)in.alive, (size_t)N));
    PML_TRY(mem.put(&d_is_tip, (const unsigned char*)in.is_tip, (size_t)N));
    PML_TRY(mem.put(&d_poly, (const unsigned char*)in.is_polytomy, (size_t)N));
    PML_TRY(mem.put(&d_up, (const int*)in.up, (size_t)N));
    PML_TRY(mem.put(&d_config, (const int*)in.config, (size_t)N));
    PML_TRY(mem.put(&d_top, (const int*)in.top, (size_t)C));
    PML_TRY(mem.put(&d_lo, (const int*)in.below_lo, (size_t)C));
    PML_TRY(mem.put(&d_hi, (const int*)in.below_hi, (size_t)C));
    PML_TRY(mem.put(&d_order, (const int*)in.tip_order, (size_t)T));
    PML_TRY(mem.put(&d_members, (const int*)in.member_offsets, (size_t)L + 1));
    PML_TRY(mem.put(&d_miles, in.milestones, (size_t)M));
    PML_TRY(mem.get(&d_get, (size_t)N));
    const size_t n_diff = (size_t)C * (M + 1);
    const int n_tiles = (T + PML_TL_TILE - 1) / PML_TL_TILE;
    const size_t n_hist = ((size_t)n_tiles + 1) * PML_TL_MAX_M;
    const size_t LM = (size_t)L * M;
    TimelineOut o;
    int** const fields[7] = {&o.n_roots, &o.tips_min, &o.tips_max, &o.internal_min, &o.internal_max, &o.below_min, &o.below_max};
    int* const host[7] = {out.n_roots, out.tips_min, out.tips_max, out.internal_min, out.internal_max, out.below_min, out.below_max};
    if (in.timeline_type == PML_TL_SAMPLED) {
        PML_TRY(mem.get(&d_smin, (size_t)N));
        PML_TRY(mem.get(&d_max, 1));
    }
    PML_TRY(mem.get(&d_bin, (size_t)N));
    PML_TRY(mem.get(&d_cbin, (size_t)N));
    PML_TRY(mem.get(&d_tbin, (size_t)T));
    PML_TRY(mem.get(&d_tips, n_diff));
    PML_TRY(mem.get(&d_internal, n_diff));
    PML_TRY(mem.get(&d_hist, n_hist));
    PML_TRY(mem.get(&d_below, (size_t)C * M));
    for (int i = 0; i < 7; ++i) PML_TRY(mem.get(fields[i], LM));
    PML_TRY(mem.get(&o.first, (size_t)L));
    PML_TRY(mem.mark());
    if (in.timeline_type == PML_TL_SAMPLED) {
        HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(tl_u64), s));
        TL_LAUNCH(tl_sampled_init_kernel, blocks, PML_TL_THREADS, N, d_date, d_alive, d_is_tip, d_smin, d_max);
        for (size_t i = runs.size(); i-- > 0;) {
            const LevelRun& r = runs[i];
            if (r.d1 <= 1) continue;   // (the roots have nothing above them)
            if (r.fused) {
                TL_LAUNCH(tl_sampled_fused_kernel, 1, PML_TL_THREADS, r.d0, r.d1, d_level, d_parent, d_smin);
            } else {
                const int a = in.level_offsets[r.d0], b = in.level_offsets[r.d1];
                TL_LAUNCH(tl_sampled_level_kernel, (b - a + PML_TL_THREADS - 1) / PML_TL_THREADS, PML_TL_THREADS, a, b, d_parent, d_smin);
            }
        }
    }
    TL_LAUNCH(tl_get_date_kernel, blocks, PML_TL_THREADS, N, in.timeline_type, d_date, d_up, d_smin, d_max, d_get);
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(out.get_date, d_get, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));

    // ---- bins -----------------------------------------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_cbin, 0x7f, (size_t)N * sizeof(int), s));
    TL_LAUNCH(tl_bins_kernel, blocks, PML_TL_THREADS, N, M, in.timeline_type, d_miles, d_date, d_get, d_alive, d_up, d_bin, d_cbin);
    TL_LAUNCH(tl_tip_bins_kernel, (T + PML_TL_THREADS - 1) / PML_TL_THREADS, PML_TL_THREADS, T, M, d_miles, d_date, d_order, d_tbin);
    PML_TRY(mem.mark());

    // ---- role counts ----------------------------------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_tips, 0, n_diff * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_internal, 0, n_diff * sizeof(int), s));
    TL_LAUNCH(tl_roles_kernel, blocks, PML_TL_THREADS, N, M, d_alive, d_config, d_is_tip, d_poly, d_bin, d_cbin, d_tips, d_internal);
    TL_LAUNCH(tl_roles_sum_kernel, (C + PML_TL_THREADS - 1) / PML_TL_THREADS, PML_TL_THREADS, C, M, d_tips, d_internal);
    PML_TRY(mem.mark());

    // ---- tips below -----------------------------------------------------------------------------------------------------
    HIP_TRY(hipMemsetAsync(d_hist, 0, n_hist * sizeof(int), s));
    TL_LAUNCH(tl_tile_hist_kernel, n_tiles, PML_TL_THREADS, T, M, d_tbin, d_hist);
    TL_LAUNCH(tl_tile_scan_kernel, 1, PML_TL_MAX_M, n_tiles, d_hist);
    TL_LAUNCH(tl_below_kernel, C, PML_TL_THREADS, M, d_lo, d_hi, d_tbin, d_hist, d_below);
    PML_TRY(mem.mark());

    // ---- vertices -------------------------------------------------------------------------------------------------------
    TL_LAUNCH(tl_vertices_kernel, L, PML_TL_THREADS, M, d_members, d_top, d_bin, d_tips, d_internal, d_below, o);
    PML_TRY(mem.mark());
    for (int i = 0; i < 7; ++i) HIP_TRY(hipMemcpyAsync(host[i], *fields[i], LM * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out.first_milestone, o.first, (size_t)L * sizeof(int), hipMemcpyDeviceToHost, s));
    PML_TRY(mem.finish());
    for (int i = 0; i < 6; ++i) {
        PML_TRY(mem.elapsed((size_t)i + (i > 0), (size_t)i + 1 + (i > 0), &ms));
        ctx->tl_ms[i] = ms;
    }
    ctx->tl_launches = launches;
    return PML_OK;
}
