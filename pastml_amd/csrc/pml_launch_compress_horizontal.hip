// Launches of one pass of the horizontal merging (pml_kernels_compress_horizontal.h): the depths and child lists of the vertex
// forest (host, O(V)), the sizes of the tables, the level loop.  pml_compress_horizontal (pml_api.hip) checks the pointers and
// W; the vertex forest itself is checked here, where it is walked anyway.
#include <climits>
#include "pml_launch.h"
#include "pml_kernels_compress_horizontal.h"

PML_INTERNAL int launch_compress_horizontal(pml_ctx* ctx, int V, int n_cols, int W, const int* parent, const int* rank, const int* bin,
                                            const int* width_in, const unsigned char* live_in, const u64* sets, int* into_out,
                                            unsigned char* live_out, int* width_out, int* groups_out) {
    // ---- the vertex forest: checks, depths, child lists (live vertices only) ----------------------------------------------
    std::vector<int> depth(V, -1), n_child(V, 0);
    long long width_total = 0;
    int n_live = 0;
    for (int v = 0; v < V; ++v) {
        if (!live_in[v]) continue;
        ++n_live;
        const int p = parent[v];
        if (p < -1 || p >= V || p == v) return fail(PML_ERR_INVALID, "parent[%d] = %d is no row of the %d vertices", v, p, V);
        if (p >= 0 && !live_in[p]) return fail(PML_ERR_INVALID, "vertex %d is live under vertex %d, which is not", v, p);
        if (bin[v] < 0) return fail(PML_ERR_INVALID, "bin[%d] = %d is negative", v, bin[v]);
        if (rank[v] < 0) return fail(PML_ERR_INVALID, "rank[%d] = %d is negative", v, rank[v]);
        if (width_in[v] < 1) return fail(PML_ERR_INVALID, "width_in[%d] = %d: the width of a live vertex is at least 1", v, width_in[v]);
        width_total += width_in[v];
        if (p >= 0) ++n_child[p];
    }
    if (width_total > INT_MAX) return fail(PML_ERR_UNSUPPORTED, "the widths sum to %lld, beyond 32 bits", width_total);
    for (int v = 0; v < V; ++v)   // (the sort pads a child list to a power of two, held in an int)
        if (n_child[v] > (1 << 30)) return fail(PML_ERR_UNSUPPORTED, "vertex %d has %d children; at most 2^30 are supported", v, n_child[v]);
    int n_levels = 0;
    {
        std::vector<int> path;
        for (int v = 0; v < V; ++v) {
            if (!live_in[v] || depth[v] >= 0) continue;
            path.clear();
            int u = v;
            while (u >= 0 && depth[u] < 0) {
                if ((int)path.size() > n_live) return fail(PML_ERR_INVALID, "the parents of the vertices form a cycle (at vertex %d)", v);
                path.push_back(u);
                u = parent[u];
            }
            int d = u < 0 ? -1 : depth[u];
            for (size_t i = path.size(); i-- > 0;) depth[path[i]] = ++d;
        }
        for (int v = 0; v < V; ++v) n_levels = std::max(n_levels, depth[v] + 1);
    }
    std::vector<int> child_off((size_t)V + 1, 0);
    for (int v = 0; v < V; ++v) child_off[v + 1] = child_off[v] + n_child[v];
    const int E = child_off[V];
    std::vector<int> child_idx(std::max(1, E));
    {
        std::vector<int> at(child_off.begin(), child_off.end() - 1);
        for (int v = 0; v < V; ++v)
            if (live_in[v] && parent[v] >= 0) child_idx[at[parent[v]]++] = v;
    }
    // per level: the vertices a lane takes, and those a workgroup takes with their runs of the sort scratch
    std::vector<int> small_off((size_t)n_levels + 1, 0), block_off((size_t)n_levels + 1, 0);
    for (int v = 0; v < V; ++v)
        if (live_in[v]) ++(n_child[v] <= PML_HZ_SMALL ? small_off : block_off)[depth[v] + 1];
    for (int d = 0; d < n_levels; ++d) {
        small_off[d + 1] += small_off[d];
        block_off[d + 1] += block_off[d];
    }
    std::vector<int> small_list(std::max(1, small_off[n_levels])), block_list(std::max(1, block_off[n_levels]));
    std::vector<long long> block_scratch(block_list.size(), -1);
    size_t scratch_words = 0;
    {
        std::vector<int> sa(small_off.begin(), small_off.end() - 1), ba(block_off.begin(), block_off.end() - 1);
        for (int v = 0; v < V; ++v) {
            if (!live_in[v]) continue;
            if (n_child[v] <= PML_HZ_SMALL) {
                small_list[sa[depth[v]]++] = v;
            } else {
                const int at = ba[depth[v]]++;
                block_list[at] = v;
                if (n_child[v] > PML_HZ_TILE) {
                    block_scratch[at] = (long long)scratch_words;
                    scratch_words += pow2_from((size_t)n_child[v]);
                }
            }
        }
    }
    // tables: twice the pairs that a pass can make, so nothing is resized or read back in its course
    const size_t pairs = (size_t)n_live * ((size_t)n_cols * W * 2 + 2) + 2 * (size_t)E;
    const size_t slots = std::max<size_t>(1024, pow2_from(2 * pairs));
    const size_t gslots = std::max<size_t>(64, pow2_from(2 * (size_t)E));
    if (slots > (1ull << 31))
        return fail(PML_ERR_UNSUPPORTED, "pml_compress_horizontal: %zu pairs need a table of more than 2^31 slots", pairs);

    // ---- device ---------------------------------------------------------------------------------------------------------
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int flags[2] = {0, 0};   // [0] a table was full, [1] groups of two or more: copied back at the end
    CallScope mem(s, ctx->profile);   // (events for pml_compress_horizontal_info only while the context profiles)
    HzTables t;
    int *d_parent, *d_rank, *d_bin, *d_width_in, *d_child_off, *d_child_idx, *d_small, *d_block, *d_width, *d_into, *d_flags;
    int *d_up[2];
    long long* d_block_scratch;
    unsigned char *d_live_in, *d_live, *d_gone[2];
    u32 *d_sclass, *d_cls, *d_slot_of;
    u64 *d_sets, *d_sort;
    const size_t n_words = (size_t)n_cols * V * W;
    PML_TRY(mem.put(&d_parent, parent, (size_t)V));
    PML_TRY(mem.put(&d_rank, rank, (size_t)V));
    PML_TRY(mem.put(&d_bin, bin, (size_t)V));
    PML_TRY(mem.put(&d_width_in, width_in, (size_t)V));
    PML_TRY(mem.put(&d_live_in, live_in, (size_t)V));
    PML_TRY(mem.put(&d_sets, sets, n_words));
    PML_TRY(mem.put(&d_child_off, child_off.data(), (size_t)V + 1));
    PML_TRY(mem.put(&d_child_idx, child_idx.data(), (size_t)E));
    PML_TRY(mem.put(&d_small, small_list.data(), (size_t)small_off[n_levels]));
    PML_TRY(mem.put(&d_block, block_list.data(), (size_t)block_off[n_levels]));
    PML_TRY(mem.put(&d_block_scratch, block_scratch.data(), (size_t)block_off[n_levels]));
    PML_TRY(mem.get(&d_width, (size_t)V));
    PML_TRY(mem.get(&d_live, (size_t)V));
    PML_TRY(mem.get(&d_into, (size_t)V));
    PML_TRY(mem.get(&d_sclass, (size_t)V));
    PML_TRY(mem.get(&d_cls, (size_t)V));
    PML_TRY(mem.get(&d_slot_of, (size_t)V));
    PML_TRY(mem.get(&d_sort, scratch_words));
    PML_TRY(mem.get(&d_flags, 2));
    for (int i = 0; i < 2; ++i) {
        PML_TRY(mem.get(&d_up[i], (size_t)V));
        PML_TRY(mem.get(&d_gone[i], (size_t)V));
    }
    PML_TRY(mem.get(&t.keys, slots));
    PML_TRY(mem.get(&t.gkeys, gslots));
    PML_TRY(mem.get(&t.gbest, gslots));
    PML_TRY(mem.get(&t.gwsum, gslots));
    t.mask = (u32)(slots - 1);
    t.gmask = (u32)(gslots - 1);
    t.error = d_flags;
    HIP_TRY(hipMemsetAsync(t.keys, 0xFF, slots * 8, s));
    HIP_TRY(hipMemsetAsync(t.gkeys, 0xFF, gslots * 8, s));
    HIP_TRY(hipMemsetAsync(t.gbest, 0xFF, gslots * 8, s));
    HIP_TRY(hipMemsetAsync(t.gwsum, 0, gslots * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_flags, 0, 2 * sizeof(int), s));
    HIP_TRY(hipMemsetAsync(d_slot_of, 0, (size_t)V * sizeof(u32), s));
    HIP_TRY(hipMemsetAsync(d_cls, 0, (size_t)V * sizeof(u32), s));
    HIP_TRY(hipMemcpyAsync(d_width, d_width_in, (size_t)V * sizeof(int), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_live, d_live_in, (size_t)V, hipMemcpyDeviceToDevice, s));
    {   // into starts as the vertex itself
        std::vector<int> self(V);
        for (int v = 0; v < V; ++v) self[v] = v;
        HIP_TRY(hipMemcpyAsync(d_into, self.data(), (size_t)V * sizeof(int), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));   // (the vector goes out of scope)
    }

    HzVertices a;
    a.parent = d_parent;
    a.rank = d_rank;
    a.bin = d_bin;
    a.width_in = d_width_in;
    a.sclass = d_sclass;
    a.child_off = d_child_off;
    a.child_idx = d_child_idx;
    a.cls = d_cls;
    a.slot_of = d_slot_of;
    a.width = d_width;
    a.live = d_live;
    a.into = d_into;
    a.groups = d_flags + 1;

    long long launches = 0;
    const int vertex_blocks = (V + PML_HZ_THREADS - 1) / PML_HZ_THREADS;
    PML_TRY(mem.mark());
    if (n_live > 0) {
        hipLaunchKernelGGL(hz_states_kernel, dim3(vertex_blocks), dim3(PML_HZ_THREADS), 0, s, t, d_sets, d_live_in, d_sclass, V, W, n_cols);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    PML_TRY(mem.mark());
    for (int d = n_levels - 1; d >= 0; --d) {
        const int ns = small_off[d + 1] - small_off[d], nb = block_off[d + 1] - block_off[d];
        if (ns > 0) {
            hipLaunchKernelGGL(hz_level_small_kernel, dim3((ns + PML_HZ_THREADS - 1) / PML_HZ_THREADS), dim3(PML_HZ_THREADS), 0, s, t, a,
                               d_small + small_off[d], ns);
            HIP_TRY(hipGetLastError());
            ++launches;
        }
        if (nb > 0) {
            hipLaunchKernelGGL(hz_level_block_kernel, dim3(nb), dim3(PML_HZ_THREADS), 0, s, t, a, d_block + block_off[d],
                               d_block_scratch + block_off[d], d_sort);
            HIP_TRY(hipGetLastError());
            ++launches;
        }
    }
    PML_TRY(mem.mark());
    // vertices under one that left leave too: 2^rounds > the deepest level
    int cur = 0;
    if (n_live > 0) {
        hipLaunchKernelGGL(hz_down_init_kernel, dim3(vertex_blocks), dim3(PML_HZ_THREADS), 0, s, d_parent, d_live_in, d_live, d_up[0],
                           d_gone[0], V);
        HIP_TRY(hipGetLastError());
        ++launches;
        for (int r = 0; (1ll << r) < n_levels; ++r) {
            hipLaunchKernelGGL(hz_down_kernel, dim3(vertex_blocks), dim3(PML_HZ_THREADS), 0, s, d_up[cur], d_gone[cur], d_up[1 - cur],
                               d_gone[1 - cur], V);
            HIP_TRY(hipGetLastError());
            ++launches;
            cur = 1 - cur;
        }
        hipLaunchKernelGGL(hz_down_finish_kernel, dim3(vertex_blocks), dim3(PML_HZ_THREADS), 0, s, d_gone[cur], d_live, V);
        HIP_TRY(hipGetLastError());
        ++launches;
    }
    PML_TRY(mem.mark());
    HIP_TRY(hipMemcpyAsync(into_out, d_into, (size_t)V * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(live_out, d_live, (size_t)V, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(width_out, d_width, (size_t)V * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(flags, d_flags, sizeof(flags), hipMemcpyDeviceToHost, s));
    PML_TRY(mem.finish());
    for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        PML_TRY(mem.elapsed(i, i + 1, &ms));
        ctx->hz_ms[i] = ms;
    }
    ctx->hz_levels = n_levels;
    ctx->hz_launches = launches;
    ctx->hz_slots = (long long)slots;
    if (flags[0]) return fail(PML_ERR_HIP, "pml_compress_horizontal: a table of %zu slots for %zu pairs was full", slots, pairs);
    if (groups_out) *groups_out = flags[1];
    return PML_OK;
}
