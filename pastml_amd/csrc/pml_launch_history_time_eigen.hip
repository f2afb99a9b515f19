// Launches of the exact dwell times, Markov jumps and lineage counts per time interval of the eigen-decomposed models
// (pml_kernels_history_time_eigen.h): the changes of basis per branch, the exponentials per segment, the pair sum over the pieces,
// the sums and transforms per bin and the lineages per boundary, for the columns [cb, ce) of the context in one go, queued on the
// context's stream.  pml_history_through_time_eigen (pml_api_readers.hip) checks the arguments, plans the segments on the host
// (pml_time_segments.h), makes sure every vector the kernels read is in HBM and copies out.
#include "pml_launch.h"
#include "pml_kernels_history_time_eigen.h"

// What the device walks, from host.plan: the pieces of the pair sum (PML_HEIG_PIECE segments, the bins proper), the flagged
// segments as a plan of their own -- still sorted by (bin, caller's id) -- and its pieces, the pseudo-bin M included.  A piece of
// the lineages is a whole number of tiles, so a boundary's tiles do not depend on the other boundaries either.
void history_time_eigen_plan(HistoryTimeEigenPlan& host) {
    static_assert(PML_HEIG_PIECE % PML_HTE_TILE == 0, "a piece of the lineages is a whole number of tiles");
    const PmlTimeSegments& plan = host.plan;
    host.pieces = pml_cut_time_pieces(plan, PML_HEIG_PIECE, false);
    PmlTimeSegments& f = host.flagged;
    f = PmlTimeSegments();
    f.M = plan.M;
    f.bin_off.assign(1, 0);
    for (int m = 0; m <= plan.M; ++m) {
        for (int i = plan.bin_off[m]; i < plan.bin_off[m + 1]; ++i) {
            if (!plan.starts[i]) continue;
            f.node.push_back(plan.node[i]);
            f.starts.push_back(1);
            f.frac.insert(f.frac.end(), plan.frac.begin() + 4 * (size_t)i, plan.frac.begin() + 4 * (size_t)i + 4);
        }
        f.bin_off.push_back(f.n_segments());
    }
    host.lpieces = pml_cut_time_pieces(f, PML_HEIG_PIECE, true);
}

PML_INTERNAL int launch_history_time_eigen(pml_ctx* ctx, CallScope& mem, int cb, int ce, const HistoryTimeEigenPlan& host,
                                           double* d_times, double* d_jumps, double* d_lineages) {
    const int k = ctx->k, N = ctx->N, cols = ce - cb, M = host.plan.M;
    if (k < 2 || k > 256) return fail(PML_ERR_UNSUPPORTED, "k = %d: the eigen models' history takes 2 to 256 states", k);
    PmlHteArgs t{};   // (what the lineages alone need stays null without them)
    PmlHeigArgs& a = t.h;
    heig_args(ctx, cb, a);   // (its pieces stay 0: the pieces are the plan's, below)
    t.M = M;
    t.n_segments = host.plan.n_interval_segments();
    t.n_pieces = host.pieces.n_pieces();
    t.n_lpieces = host.lpieces.n_pieces();
    t.times_out = d_times;
    t.jumps_out = d_jumps;
    t.lineages_out = d_lineages;
    const size_t kk = (size_t)k * k, S = (size_t)t.n_segments;
    int *d_node, *d_piece_off, *d_bin_piece_off;
    double* d_frac;
    PML_TRY(mem.put(&d_node, host.plan.node.data(), S));
    PML_TRY(mem.put(&d_frac, host.plan.frac.data(), 4 * S));
    PML_TRY(mem.put(&d_piece_off, host.pieces.piece_off.data(), host.pieces.piece_off.size()));
    PML_TRY(mem.put(&d_bin_piece_off, host.pieces.bin_piece_off.data(), host.pieces.bin_piece_off.size()));
    t.seg_node = d_node;
    t.seg_frac = d_frac;
    t.piece_off = d_piece_off;
    t.bin_piece_off = d_bin_piece_off;
    PML_TRY(mem.get(&a.stage, (size_t)cols * N * 3 * ctx->ks));
    PML_TRY(mem.get(&a.tprime, (size_t)cols * N));
    PML_TRY(mem.get(&t.sstage, (size_t)cols * S * 3 * ctx->ks));
    PML_TRY(mem.get(&t.sy, (size_t)cols * S));
    PML_TRY(mem.get(&t.partial, (size_t)cols * t.n_pieces * kk));
    PML_TRY(mem.get(&t.Wsum, (size_t)cols * M * kk));
    PML_TRY(mem.get(&t.T1, (size_t)cols * M * kk));
    launch_heig_basis(ctx, cols, a);
    if (t.n_pieces > 0) {
        hipLaunchKernelGGL(hte_segment_kernel, dim3((unsigned)((S * k + 255) / 256), cols), dim3(256), 0, ctx->stream, t);
        with_heig_rows(k, [&](auto CR) {
            hipLaunchKernelGGL(hte_pair_kernel<CR()>, dim3(t.n_pieces, a.tc * a.td, cols), dim3(256), 0, ctx->stream, t);
        });
    }
    const dim3 square((unsigned)(M * ((kk + 255) / 256)), cols);
    hipLaunchKernelGGL(hte_reduce_kernel, square, dim3(256), 0, ctx->stream, t);
    hipLaunchKernelGGL(hte_t1_kernel, square, dim3(256), 0, ctx->stream, t);
    hipLaunchKernelGGL(hte_times_kernel, dim3(M, cols), dim3(256), 0, ctx->stream, t);
    if (d_jumps != nullptr) hipLaunchKernelGGL(hte_jumps_kernel, square, dim3(256), 0, ctx->stream, t);
    if (d_lineages != nullptr) {
        int *d_lnode, *d_lpiece_off, *d_bin_lpiece_off;
        double* d_lfrac;
        PML_TRY(mem.put(&d_lnode, host.flagged.node.data(), host.flagged.node.size()));
        PML_TRY(mem.put(&d_lfrac, host.flagged.frac.data(), host.flagged.frac.size()));
        PML_TRY(mem.put(&d_lpiece_off, host.lpieces.piece_off.data(), host.lpieces.piece_off.size()));
        PML_TRY(mem.put(&d_bin_lpiece_off, host.lpieces.bin_piece_off.data(), host.lpieces.bin_piece_off.size()));
        t.lin_node = d_lnode;
        t.lin_frac = d_lfrac;
        t.lpiece_off = d_lpiece_off;
        t.bin_lpiece_off = d_bin_lpiece_off;
        PML_TRY(mem.get(&t.lpart, (size_t)cols * t.n_lpieces * k));
        if (t.n_lpieces > 0) {
            const int kp = (k + 15) & ~15;
            const size_t llds = (size_t)(16 * (kp + 1) + 48) * sizeof(double) + 16 * sizeof(int);
            const dim3 lgrid(t.n_lpieces, cols);
            if (k >= 16) hipLaunchKernelGGL(hte_lineage_kernel<true>, lgrid, dim3(256), llds, ctx->stream, t);
            else hipLaunchKernelGGL(hte_lineage_kernel<false>, lgrid, dim3(256), llds, ctx->stream, t);
        }
        hipLaunchKernelGGL(hte_lineage_sum_kernel, dim3(M + 1, cols), dim3(256), 0, ctx->stream, t);
    }
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
