// Launches of the trimming (pml_kernels_compress_trim.h): the checks of the vertex forest with its depths and subtree sizes
// (host, O(L)), the rounds of the multiplier, the thresholds -- the k-th largest candidate of every tree, taken on the host
// from one download of the candidate values: the one scalar per tree that everything after it depends on --, the scan, the
// chains.  pml_compress_trim (pml_api.hip) checks the pointers and W.
#include <cmath>
#include <functional>
#include <limits>
#include "pml_launch.h"
#include "pml_kernels_compress_trim.h"

PML_INTERNAL int launch_compress_trim(pml_ctx* ctx, int L, int n_cols, int W, const int* parent, const int* tree, const int* T,
                                      const int* w, const u64* sets, int tip_size_threshold, int n_trees,
                                      const unsigned char* trim_tree, double* tsize_out, unsigned char* keep_out,
                                      unsigned char* spliced_out, int* new_parent_out, unsigned char* moved_out, double* threshold_out) {
    // ---- the vertex forest: checks, levels, subtree sizes ---------------------------------------------------------------------
    std::vector<int> depth(L), size(L, 1);
    int n_levels = 0;
    bool any = false;
    for (int i = 0; i < L; ++i) {
        const int p = parent[i];
        if (p < -1 || p >= i) return fail(PML_ERR_INVALID, "parent[%d] = %d: the entries are in pre-order, a parent comes before its children", i, p);
        if (w[i] < 1) return fail(PML_ERR_INVALID, "w[%d] = %d: a width is at least 1", i, w[i]);
        if (T[i] < 0) return fail(PML_ERR_INVALID, "T[%d] = %d is negative", i, T[i]);
        if (tree[i] < 0 || tree[i] >= n_trees) return fail(PML_ERR_INVALID, "tree[%d] = %d is none of the %d trees", i, tree[i], n_trees);
        if (p >= 0 && tree[p] != tree[i]) return fail(PML_ERR_INVALID, "entry %d and its parent %d are in different trees", i, p);
        depth[i] = p < 0 ? 0 : depth[p] + 1;
        n_levels = std::max(n_levels, depth[i] + 1);
        any = any || trim_tree[tree[i]];
    }
    for (int i = L - 1; i >= 0; --i)
        if (parent[i] >= 0) size[parent[i]] += size[i];
    for (int i = 0; i < L; ++i)   // (with this every subtree is the run [i, i + size[i]), and it ends inside the L entries)
        if (parent[i] >= 0 && (long long)i + size[i] > (long long)parent[i] + size[parent[i]])
            return fail(PML_ERR_INVALID, "the entries are not in pre-order: the subtree of entry %d is no run of consecutive entries", parent[i]);
    int rounds = 0;
    while ((1ll << rounds) < n_levels) ++rounds;

    for (int i = 0; i < L; ++i) {   // what holds where nothing is trimmed
        tsize_out[i] = 0.;
        keep_out[i] = 1;
        spliced_out[i] = 0;
        new_parent_out[i] = parent[i];
        moved_out[i] = 0;
    }
    for (int t = 0; t < n_trees; ++t) threshold_out[t] = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < 3; ++i) ctx->trim_ms[i] = 0;
    ctx->trim_levels = n_levels;
    ctx->trim_rounds = 0;
    ctx->trim_launches = 0;
    if (!any) return PML_OK;

    // ---- device ---------------------------------------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    std::vector<double> candidate(L);           // (host buffers of asynchronous copies: declared before the scope)
    std::vector<unsigned char> trimmed(n_trees, 0);
    int error = 0;
    CallScope mem(s, ctx->profile);   // (events for pml_compress_trim_info only while the context profiles)
    TrimForest f;
    int *d_parent, *d_tree, *d_T, *d_w, *d_size, *d_up[2], *d_error, *d_tile, *d_incl, *d_n_kept, *d_only, *d_new_parent;
    unsigned char *d_gate, *d_trimmed, *d_keep, *d_spliced, *d_moved;
    double *d_mult[2], *d_tsize, *d_candidate, *d_threshold;
    unsigned long long* d_child_max;
    u64* d_sets;
    const int n_tiles = (L + PML_TRIM_TILE - 1) / PML_TRIM_TILE;
    PML_TRY(mem.put(&d_parent, parent, (size_t)L));
    PML_TRY(mem.put(&d_tree, tree, (size_t)L));
    PML_TRY(mem.put(&d_T, T, (size_t)L));
    PML_TRY(mem.put(&d_w, w, (size_t)L));
    PML_TRY(mem.put(&d_size, (const int*)size.data(), (size_t)L));
    PML_TRY(mem.put(&d_gate, trim_tree, (size_t)n_trees));
    for (int i = 0; i < 2; ++i) {
        PML_TRY(mem.get(&d_up[i], (size_t)L));
        PML_TRY(mem.get(&d_mult[i], (size_t)L));
    }
    PML_TRY(mem.get(&d_tsize, (size_t)L));
    PML_TRY(mem.get(&d_candidate, (size_t)L));
    PML_TRY(mem.get(&d_child_max, (size_t)L));
    PML_TRY(mem.get(&d_error, 1));
    HIP_TRY(hipMemsetAsync(d_child_max, 0, (size_t)L * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(d_error, 0, sizeof(int), s));
    f.parent = d_parent;
    f.tree = d_tree;
    f.T = d_T;
    f.w = d_w;
    f.size = d_size;
    f.on = d_gate;
    f.L = L;

    long long launches = 0;
    const int blocks = (L + PML_TRIM_THREADS - 1) / PML_TRIM_THREADS;
    PML_TRY(mem.mark());
    hipLaunchKernelGGL(trim_mult_init_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, f, d_mult[0], d_up[0]);
    HIP_TRY(hipGetLastError());
    ++launches;
    int cur = 0;
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(trim_mult_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, d_mult[cur], d_up[cur], d_mult[1 - cur],
                           d_up[1 - cur], L);
        HIP_TRY(hipGetLastError());
        ++launches;
        cur = 1 - cur;
    }
    hipLaunchKernelGGL(trim_tsize_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, f, d_mult[cur], d_tsize, d_child_max, d_error);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trim_candidates_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, f, d_tsize, d_child_max, d_candidate);
    HIP_TRY(hipGetLastError());
    launches += 2;
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(candidate.data(), d_candidate, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(tsize_out, d_tsize, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&error, d_error, sizeof(int), hipMemcpyDeviceToHost, s));
    PML_TRY(mem.finish());
    ctx->trim_rounds = rounds;
    ctx->trim_launches = launches;
    if (error) {
        for (int i = 0; i < L; ++i) tsize_out[i] = 0.;
        return fail(PML_ERR_UNSUPPORTED, "pml_compress_trim: the widths along a path multiply to 2^53 or more; sizes beyond the exact "
                                         "range of float64 are not supported");
    }

    // ---- thresholds: sorted(candidates)[-k] per tree, unless the smallest candidate is no smaller ---------------------------------
    bool some = false;
    {
        std::vector<std::vector<double>> of_tree(n_trees);
        for (int i = 0; i < L; ++i)
            if (candidate[i] >= 0.) of_tree[tree[i]].push_back(candidate[i]);
        for (int t = 0; t < n_trees; ++t) {
            std::vector<double>& v = of_tree[t];
            if (!trim_tree[t] || v.empty()) continue;
            const double smallest = *std::min_element(v.begin(), v.end());
            double chosen = smallest;   // (k = 0 reads sorted(...)[0])
            if (tip_size_threshold > 0 && (size_t)tip_size_threshold <= v.size()) {
                std::nth_element(v.begin(), v.begin() + (tip_size_threshold - 1), v.end(), std::greater<double>());
                chosen = v[tip_size_threshold - 1];
            }
            if (smallest < chosen) {
                threshold_out[t] = chosen;
                trimmed[t] = 1;
                some = true;
            }
        }
    }
    float ms = 0.f;
    PML_TRY(mem.elapsed(0, 1, &ms));
    ctx->trim_ms[0] = ms;
    if (!some) return PML_OK;

    // ---- removal --------------------------------------------------------------------------------------------------------
    const size_t n_words = (size_t)n_cols * L * W;
    PML_TRY(mem.put(&d_trimmed, (const unsigned char*)trimmed.data(), (size_t)n_trees));
    PML_TRY(mem.put(&d_threshold, (const double*)threshold_out, (size_t)n_trees));
    PML_TRY(mem.put(&d_sets, sets, n_words));
    PML_TRY(mem.get(&d_tile, (size_t)n_tiles));
    PML_TRY(mem.get(&d_incl, (size_t)L));
    PML_TRY(mem.get(&d_n_kept, (size_t)L));
    PML_TRY(mem.get(&d_only, (size_t)L));
    PML_TRY(mem.get(&d_new_parent, (size_t)L));
    PML_TRY(mem.get(&d_keep, (size_t)L));
    PML_TRY(mem.get(&d_spliced, (size_t)L));
    PML_TRY(mem.get(&d_moved, (size_t)L));
    HIP_TRY(hipMemsetAsync(d_n_kept, 0, (size_t)L * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_only, 0, (size_t)L * sizeof(int), s));   // (entry 0 where no child survives: a valid index)
    HIP_TRY(hipMemsetAsync(d_spliced, 0, (size_t)L, s));
    f.on = d_trimmed;
    PML_TRY(mem.mark());
    hipLaunchKernelGGL(trim_scan_totals_kernel, dim3(n_tiles), dim3(PML_TRIM_THREADS), 0, s, f, d_tsize, d_threshold, d_tile);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trim_scan_tiles_kernel, dim3(1), dim3(PML_TRIM_THREADS), 0, s, d_tile, n_tiles);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trim_scan_write_kernel, dim3(n_tiles), dim3(PML_TRIM_THREADS), 0, s, f, d_tsize, d_threshold, d_tile, d_incl);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trim_keep_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, f, d_tsize, d_threshold, d_incl, d_keep, d_n_kept,
                       d_only);
    HIP_TRY(hipGetLastError());
    launches += 4;
    PML_TRY(mem.mark());

    // ---- mediators ------------------------------------------------------------------------------------------------------
    const int WG = (int)pow2_from((size_t)W);
    const int per_block = PML_TRIM_THREADS / WG;
    hipLaunchKernelGGL(trim_chain_kernel, dim3((L + per_block - 1) / per_block), dim3(PML_TRIM_THREADS), 0, s, f, d_sets, d_keep, d_n_kept,
                       d_only, d_spliced, W, WG, n_cols);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(trim_parents_kernel, dim3(blocks), dim3(PML_TRIM_THREADS), 0, s, f, d_keep, d_spliced, d_new_parent, d_moved);
    HIP_TRY(hipGetLastError());
    launches += 2;
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(keep_out, d_keep, (size_t)L, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(spliced_out, d_spliced, (size_t)L, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(new_parent_out, d_new_parent, (size_t)L * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(moved_out, d_moved, (size_t)L, hipMemcpyDeviceToHost, s));
    PML_TRY(mem.finish());
    PML_TRY(mem.elapsed(2, 3, &ms));
    ctx->trim_ms[1] = ms;
    PML_TRY(mem.elapsed(3, 4, &ms));
    ctx->trim_ms[2] = ms;
    ctx->trim_launches = launches;
    return PML_OK;
}
