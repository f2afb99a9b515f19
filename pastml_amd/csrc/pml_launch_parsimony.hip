// Launches of the parsimony passes (pml_kernels_parsimony.h): the chunks of columns, the level schedule of every pass; the
// scratch and the event brackets live in a CallScope (pml_call_scope.h).  pml_parsimony (pml_api.hip) checks the arguments.
#include "pml_launch.h"
#include "pml_kernels_parsimony.h"

// Scratch per column, in units of N W 8 bytes: staging in the caller's numbering, starting sets, bottom-up sets, "up" sets, the
// sets of the method at hand, Z of the step count -- 6 -- plus N int64 costs (1 / W): at most 7.
#define PML_PARS_SETS_PER_COLUMN 6

namespace {

struct ParsRun {
    pml_ctx* ctx;
    PmlParsArgs a;
    int planes;        // of the bit-sliced counters: 2^planes > largest number of children + 1
    int thin;          // levels of at most this many units share a launch of one workgroup per column
    int cols;          // of the chunk
    long long launches = 0;
    const int *d_bu_offsets, *d_td_offsets, *d_tdp_offsets;
};

template <int PASS, int P>
static int launch_levels(ParsRun& r, const PmlParsArgs& a, int l0, int l1, int blocks) {
    hipLaunchKernelGGL((pars_levels_kernel<PASS, P>), dim3(blocks, r.cols), dim3(PML_PARS_THREADS), 0, r.ctx->stream, a, l0, l1);
    HIP_TRY(hipGetLastError());
    ++r.launches;
    return PML_OK;
}

template <int PASS>
static int launch_levels_p(ParsRun& r, const PmlParsArgs& a, int l0, int l1, int blocks) {
    if (PASS == PML_PARS_RESTRICT) return launch_levels<PASS, 2>(r, a, l0, l1, blocks);   // (no counters)
    switch (r.planes) {
        case 2: return launch_levels<PASS, 2>(r, a, l0, l1, blocks);
        case 4: return launch_levels<PASS, 4>(r, a, l0, l1, blocks);
        case 8: return launch_levels<PASS, 8>(r, a, l0, l1, blocks);
        case 16: return launch_levels<PASS, 16>(r, a, l0, l1, blocks);
        default: return launch_levels<PASS, 32>(r, a, l0, l1, blocks);
    }
}

// one pass over the levels of `offsets` (host copy of a.offsets): runs of thin levels in one launch, a wide level in its own
template <int PASS>
static int run_pass(ParsRun& r, const PmlParsArgs& a, const std::vector<int>& offsets) {
    const int L = (int)offsets.size() - 1;
    const int per_block = PML_PARS_THREADS / a.WG;
    for (int l = 0; l < L;) {
        const int n = offsets[l + 1] - offsets[l];
        if (n <= r.thin) {
            int e = l + 1;
            while (e < L && offsets[e + 1] - offsets[e] <= r.thin) ++e;
            PML_TRY(launch_levels_p<PASS>(r, a, l, e, 1));
            l = e;
        } else {
            const int blocks = std::min((n + per_block - 1) / per_block, 8192);
            PML_TRY(launch_levels_p<PASS>(r, a, l, l + 1, blocks));
            ++l;
        }
    }
    return PML_OK;
}

}  // namespace

PML_INTERNAL int launch_parsimony(pml_ctx* ctx, int n_cols, int k, const u64* given, int methods, u64* sets_out, i64* steps_out,
                                  i64* hist_out) {
    const PmlForest& f = ctx->forest;
    const int N = ctx->N, W = (k + 63) / 64;
    const int WG = (int)pow2_from((size_t)W);
    int maxc = 0;
    for (int i = 0; i < N; ++i) maxc = std::max(maxc, f.n_children[i]);
    int planes = 2;
    while (planes < 32 && (1ll << planes) <= (long long)maxc + 1) planes <<= 1;
    int n_methods = 0;
    for (int b = 0; b < 3; ++b) n_methods += (methods >> b) & 1;
    const size_t col_words = (size_t)N * W, hist_len = (size_t)k + 1;

    // columns per chunk: what the scratch allows (half of the free memory at most)
    const size_t per_col = col_words * 8 * PML_PARS_SETS_PER_COLUMN + (size_t)N * 8 + 3 * (hist_len + 1) * 8;
    long long chunk;
    PML_TRY(columns_per_chunk(ctx, per_col, 65535, T_PARS_MAX_COLS, n_cols, "pml_parsimony", &chunk));

    hipStream_t s = ctx->stream;
    CallScope mem(s, true);   // (events always: pml_parsimony_info reports the passes' time whether or not the context profiles)
    u64 *d_stage, *d_init, *d_bu, *d_up, *d_out, *d_z, *d_steps, *d_hist;
    i64* d_m;
    int* d_tdp_offsets;
    PML_TRY(mem.get(&d_stage, chunk * col_words));
    PML_TRY(mem.get(&d_init, chunk * col_words));
    PML_TRY(mem.get(&d_bu, chunk * col_words));
    PML_TRY(mem.get(&d_up, chunk * col_words));
    PML_TRY(mem.get(&d_out, chunk * col_words));
    PML_TRY(mem.get(&d_z, chunk * col_words));
    PML_TRY(mem.get(&d_m, (size_t)chunk * N));
    PML_TRY(mem.get(&d_steps, (size_t)3 * chunk));
    PML_TRY(mem.get(&d_hist, (size_t)3 * chunk * hist_len));
    PML_TRY(mem.put(&d_tdp_offsets, f.td_parent_offsets.data(), f.td_parent_offsets.size()));

    ParsRun r;
    r.ctx = ctx;
    r.planes = planes;
    r.thin = (int)std::max(1ll, ctx->tune.get(T_PARS_THIN, 512));
    PmlParsArgs base;
    base.parent = ctx->d_parent;
    base.first_child = ctx->d_first_child;
    base.n_children = ctx->d_n_children;
    base.list = nullptr;
    base.offsets = nullptr;
    base.N = N;
    base.W = W;
    base.WG = WG;
    base.last_word = (k % 64) ? ((1ull << (k % 64)) - 1) : ~0ull;
    base.init = d_init;
    base.src = nullptr;
    base.dst = nullptr;
    base.up = d_up;
    base.m = d_m;
    const bool perm = !ctx->old_of_new.empty();
    const int first_root = f.td_offsets[0], n_roots = f.td_offsets[1] - f.td_offsets[0];
    double pass_ms = 0;

    for (int c0 = 0; c0 < n_cols; c0 += (int)chunk) {
        const int cc = std::min<int>((int)chunk, n_cols - c0);
        const size_t words = (size_t)cc * col_words;
        const int flat_blocks = (int)std::min<size_t>(((size_t)cc * N + 255) / 256, 16384);
        r.cols = cc;
        std::vector<size_t> pass_seg;   // indices i of the event pairs (i, i + 1) that bracket passes
        HIP_TRY(hipMemcpyAsync(d_stage, given + (size_t)c0 * col_words, words * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_steps, 0, (size_t)3 * cc * 8, s));
        HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)3 * cc * hist_len * 8, s));
        PML_TRY(mem.mark());
        pass_seg.push_back(mem.n_marks() - 1);
        hipLaunchKernelGGL(pars_init_kernel, dim3(flat_blocks), dim3(256), 0, s, d_stage, d_init, perm ? ctx->d_old_of_new : nullptr, N, W,
                           base.last_word, cc);
        HIP_TRY(hipGetLastError());
        ++r.launches;
        HIP_TRY(hipMemcpyAsync(d_bu, d_init, words * 8, hipMemcpyDeviceToDevice, s));
        {
            PmlParsArgs a = base;
            a.list = ctx->d_bu_order;
            a.offsets = ctx->d_bu_offsets;
            a.dst = d_bu;
            PML_TRY(run_pass<PML_PARS_UP>(r, a, f.bu_offsets));
        }
        int slot = 0;
        // the sets of one method are in d_out: sizes, steps, then out in the caller's numbering
        auto finish = [&]() -> int {
            hipLaunchKernelGGL(pars_hist_kernel, dim3(std::min((N + 255) / 256, 256), cc), dim3(256), hist_len * sizeof(int), s, d_out,
                               d_hist + (size_t)slot * cc * hist_len, N, W, k);
            HIP_TRY(hipGetLastError());
            ++r.launches;
            HIP_TRY(hipMemcpyAsync(d_z, d_out, words * 8, hipMemcpyDeviceToDevice, s));   // tips: Z = the set, cost 0
            HIP_TRY(hipMemsetAsync(d_m, 0, (size_t)cc * N * 8, s));
            PmlParsArgs a = base;
            a.list = ctx->d_bu_order;
            a.offsets = ctx->d_bu_offsets;
            a.src = d_out;
            a.dst = d_z;
            PML_TRY(run_pass<PML_PARS_STEPS>(r, a, f.bu_offsets));
            hipLaunchKernelGGL(pars_root_steps_kernel, dim3(std::min((n_roots + 255) / 256, 64), cc), dim3(256), 0, s, d_m,
                               d_steps + (size_t)slot * cc, N, first_root, n_roots);
            HIP_TRY(hipGetLastError());
            ++r.launches;
            PML_TRY(mem.mark());
            hipLaunchKernelGGL(pars_gather_kernel, dim3(flat_blocks), dim3(256), 0, s, d_out, d_stage, perm ? ctx->d_new_of_old : nullptr,
                               N, W, cc);
            HIP_TRY(hipGetLastError());
            ++r.launches;
            HIP_TRY(hipMemcpyAsync(sets_out + ((size_t)slot * n_cols + c0) * col_words, d_stage, words * 8, hipMemcpyDeviceToHost, s));
            PML_TRY(mem.mark());
            pass_seg.push_back(mem.n_marks() - 1);
            ++slot;
            return PML_OK;
        };
        if (methods & 1) {   // ACCTRAN
            PmlParsArgs a = base;
            a.offsets = ctx->d_td_offsets;
            a.src = d_bu;
            a.dst = d_out;
            PML_TRY(run_pass<PML_PARS_RESTRICT>(r, a, f.td_offsets));
            PML_TRY(finish());
        }
        if (methods & 6) {
            HIP_TRY(hipMemcpyAsync(d_out, d_init, words * 8, hipMemcpyDeviceToDevice, s));   // (a tree that is one tip keeps its set)
            PmlParsArgs a = base;
            a.list = ctx->d_td_parents;
            a.offsets = d_tdp_offsets;
            a.src = d_bu;
            a.dst = d_out;
            PML_TRY(run_pass<PML_PARS_DOWN>(r, a, f.td_parent_offsets));
            if (methods & 2) PML_TRY(finish());
            if (methods & 4) {   // DELTRAN: on the DOWNPASS sets, in place (a node reads its parent's new set)
                PmlParsArgs b = base;
                b.offsets = ctx->d_td_offsets;
                b.src = d_out;
                b.dst = d_out;
                PML_TRY(run_pass<PML_PARS_RESTRICT>(r, b, f.td_offsets));
                PML_TRY(finish());
            }
        }
        PML_TRY(mem.mark());
        for (int m = 0; m < n_methods; ++m) {
            HIP_TRY(hipMemcpyAsync(steps_out + (size_t)m * n_cols + c0, d_steps + (size_t)m * cc, (size_t)cc * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(hist_out + ((size_t)m * n_cols + c0) * hist_len, d_hist + (size_t)m * cc * hist_len,
                                   (size_t)cc * hist_len * 8, hipMemcpyDeviceToHost, s));
        }
        PML_TRY(mem.finish());
        for (size_t i : pass_seg) {
            float ms = 0.f;
            PML_TRY(mem.elapsed(i, i + 1, &ms));
            pass_ms += ms;
        }
    }
    ctx->pars_launches = r.launches;
    ctx->pars_ms = pass_ms;
    return PML_OK;
}
