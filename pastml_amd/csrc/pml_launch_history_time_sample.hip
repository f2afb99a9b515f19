// Launches of the history sampler per time interval (pml_kernels_history_time_sample.h) for one column: the upload of the
// plan, launch_scenarios, whose states the walk reads from the device, the count of the branches that cannot be drawn, the walk
// over (piece of segments, tile of repetitions) items and the sum of the pieces' partials per bin, queued on the context's
// stream.  The plan goes up first, so that its copies from pageable memory are not queued behind the scenario kernels.
// pml_sample_histories_through_time (pml_api_readers.hip) checks the arguments, plans the segments on the host (pml_time_segments.h),
// makes sure every vector the kernels read is in HBM, zeroes the counters and copies out.
#include "pml_launch.h"
#include "pml_kernels_history_time_sample.h"

// Segments per piece: the ids per piece of pml_launch_history_sample.hip, 64 ceil(max(64, ceil(N / 256)) / 64) -- fixed by N,
// never by the grid, by k or by the bins (the sums' order, hence their bits, follows from it).  The pieces are cut per bin
// (pml_cut_time_pieces): at most 256 + M + (segments - N) / piece of them.
int history_time_sample_piece(int N) { return 64 * ((std::max(64, (N + 255) / 256) + 63) / 64); }

#define PML_HTSAMP_LDS_BYTES (136 * 1024)   // of the 160 KiB of a CU, as pml_launch_history_sample.hip

// Repetitions per workgroup (one per thread): the largest of 256, 128 and 64 whose accumulators fit, as hsamp_tile.
static int htsamp_tile(int k, int n_rep) {
    int T = 64;
    for (int t : {128, 256})
        if (((size_t)k * (t + 1) + 2 * (size_t)k) * sizeof(double) <= PML_HTSAMP_LDS_BYTES) T = t;
    return std::min(T, 64 * ((n_rep + 63) / 64));
}

PML_INTERNAL int launch_history_time_sample(pml_ctx* ctx, CallScope& mem, int col, int n_rep, int rep_offset, u64 seed,
                                            void* d_states, size_t rs, HistoryTimeSamplePlan& host, double* d_times,
                                            unsigned* d_jumps, unsigned* d_lineages, unsigned long long* d_fallback,
                                            unsigned long long* d_skipped) {
    const PmlTimeSegments& plan = host.plan;
    const PmlTimeSegmentEnds& ends = host.ends;
    const PmlTimePieces& pieces = host.pieces;
    const int k = ctx->k, N = ctx->N, M = plan.M;
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    const bool wide = k > PML_HSAMP_LDS_K;
    PmlHtsampArgs a;
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
    a.M = M;
    // the pieces that are walked: those of the bins proper and, if the lineages are asked for, of the pseudo-bin behind them
    const int n_bins = (int)pieces.bin_piece_off.size() - 1;   // M, or M + 1 with the pseudo-bin
    a.n_sum_pieces = pieces.bin_piece_off[M];
    a.n_pieces = d_lineages != nullptr ? pieces.n_pieces() : a.n_sum_pieces;
    const size_t S = (size_t)plan.n_segments();
    std::vector<int>&flags = host.flags, &piece_bin = host.piece_bin;
    std::vector<double>& pos = host.pos;
    flags.resize(S);
    piece_bin.resize((size_t)pieces.n_pieces());
    pos.resize(3 * S);
    for (size_t i = 0; i < S; ++i) {
        flags[i] = (plan.starts[i] ? PML_HTSAMP_STARTS : 0) | (ends.ends[i] ? PML_HTSAMP_ENDS : 0);
        pos[3 * i] = plan.frac[4 * i];
        pos[3 * i + 1] = plan.frac[4 * i + 1];
        pos[3 * i + 2] = ends.s2[i];
    }
    for (int m = 0; m < n_bins; ++m)
        for (int j = pieces.bin_piece_off[m]; j < pieces.bin_piece_off[m + 1]; ++j) piece_bin[(size_t)j] = m;
    int *d_node, *d_flags, *d_piece_off, *d_piece_bin, *d_bin_piece_off;
    double* d_pos;
    PML_TRY(mem.put(&d_node, plan.node.data(), plan.node.size()));
    PML_TRY(mem.put(&d_flags, flags.data(), flags.size()));
    PML_TRY(mem.put(&d_pos, pos.data(), pos.size()));
    PML_TRY(mem.put(&d_piece_off, pieces.piece_off.data(), pieces.piece_off.size()));
    PML_TRY(mem.put(&d_piece_bin, piece_bin.data(), piece_bin.size()));
    PML_TRY(mem.put(&d_bin_piece_off, pieces.bin_piece_off.data(), (size_t)M + 1));
    a.seg_node = d_node;
    a.seg_flags = d_flags;
    a.seg_pos = d_pos;
    a.piece_off = d_piece_off;
    a.piece_bin = d_piece_bin;
    a.bin_piece_off = d_bin_piece_off;
    const int T = wide ? 64 : htsamp_tile(k, n_rep);
    a.n_tiles = (n_rep + T - 1) / T;
    a.n_rep = n_rep;
    a.rs = rs;
    a.states = d_states;
    a.rep_offset = (unsigned)rep_offset;
    a.seed = seed;
    a.times_out = d_times;
    a.jumps = d_jumps;
    a.lineages = d_lineages;
    a.n_skipped = d_skipped;
    const size_t n_partial = (size_t)a.n_sum_pieces * n_rep * k;
    PML_TRY(mem.get(&a.partial, std::max<size_t>(n_partial, 1)));
    const long long items = (long long)a.n_pieces * a.n_tiles;
    if (items > 0x7fffffffll)
        return fail(PML_ERR_INVALID, "pml_sample_histories_through_time: %lld work items; draw fewer repetitions per call", items);
    PML_TRY(launch_scenarios(ctx, col, n_rep, rep_offset, seed, d_states, rs, d_fallback));
    hipLaunchKernelGGL(htsamp_count_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    if (items > 0) {
        if (wide) {
            // the accumulators are the partials themselves
            HIP_TRY(hipMemsetAsync(a.partial, 0, std::max<size_t>(n_partial, 1) * sizeof(double), ctx->stream));
            hipLaunchKernelGGL(htsamp_kernel<true>, dim3((unsigned)items), dim3(T), (size_t)2 * k * sizeof(double), ctx->stream, a);
        } else {
            const size_t lds = ((size_t)k * (T + 1) + 2 * (size_t)k) * sizeof(double);   // (at most PML_HTSAMP_LDS_BYTES)
            if (lds > 64 * 1024) PML_TRY(with_lds(ctx, htsamp_kernel<false>, lds));
            hipLaunchKernelGGL(htsamp_kernel<false>, dim3((unsigned)items), dim3(T), lds, ctx->stream, a);
        }
        HIP_TRY(hipGetLastError());
    }
    const size_t total = (size_t)n_rep * M * k;
    hipLaunchKernelGGL(htsamp_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
