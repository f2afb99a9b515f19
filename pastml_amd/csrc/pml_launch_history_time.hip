// Launches of the exact dwell times, Markov jumps and lineage counts per time interval of the F81 family
// (pml_kernels_history_time.h): the segment pass, the jump product and the sums of the partials per bin, for the columns
// [cb, ce) of the context in one go, queued on the context's stream.  pml_history_through_time (pml_api_readers.hip) checks the
// arguments, plans the segments on the host (pml_time_segments.h), makes sure every vector the kernels read is in HBM and
// copies out.
#include "pml_launch.h"
#include "pml_kernels_history_time.h"

// Segments per piece: fixed by k, never by the grid or by the bins (the sums' order, hence their bits, follows from it); the
// pieces are cut per bin (pml_cut_time_pieces).  The sizes of pml_launch_history.hip, for its reasons: a segment streams what a
// branch streams there.
int history_time_piece(int k) { return k <= 4 ? 1024 : (k <= 64 ? 512 : 256); }
int history_time_jump_piece(int k) { return k <= 64 ? 2048 : 4096; }

PML_INTERNAL int launch_history_time(pml_ctx* ctx, CallScope& mem, int cb, int ce, const PmlTimeSegments& plan, const PmlTimePieces& pieces,
                                     const PmlTimePieces& jpieces, double* d_times, double* d_jumps, double* d_lineages) {
    const int k = ctx->k, cols = ce - cb, M = plan.M;
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    PmlHistTimeArgs t;
    PmlHistArgs& a = t.h;
    a.parent = ctx->d_parent;
    a.n_children = ctx->d_n_children;
    a.new_of_old = ctx->d_new_of_old;   // (null when the library works in the caller's numbering)
    a.dist = ctx->d_dist;
    a.masks = ctx->d_masks;
    a.pi = ctx->d_pi;
    a.bu = ctx->d_bu;
    a.post = ctx->d_post;
    a.E = ctx->d_E;
    a.mu = ctx->d_mu;
    a.sf = ctx->d_sf;
    a.tau = ctx->d_tau;
    a.tauf = ctx->d_tauf;
    a.N = ctx->N;
    a.k = k;
    a.ks = ctx->ks;
    a.W = ctx->W;
    a.col0 = cb;
    a.piece = a.n_pieces = a.jpiece = a.n_jpieces = 0;   // (the pieces are the plan's, below)
    a.partial = a.stage = a.jpartial = a.xa = a.times_out = a.branch_out = a.jumps_out = nullptr;
    t.M = M;
    t.n_segments = plan.n_segments();
    t.n_pieces = pieces.n_pieces();
    t.n_jpieces = jpieces.n_pieces();
    t.times_out = d_times;
    t.jumps_out = d_jumps;
    t.lineages_out = d_lineages;
    t.stage = t.jpartial = nullptr;
    t.jpiece_off = t.bin_jpiece_off = nullptr;
    int *d_node, *d_starts, *d_piece_off, *d_bin_piece_off;
    double* d_frac;
    PML_TRY(mem.put(&d_node, plan.node.data(), plan.node.size()));
    PML_TRY(mem.put(&d_starts, plan.starts.data(), plan.starts.size()));
    PML_TRY(mem.put(&d_frac, plan.frac.data(), plan.frac.size()));
    PML_TRY(mem.put(&d_piece_off, pieces.piece_off.data(), pieces.piece_off.size()));
    PML_TRY(mem.put(&d_bin_piece_off, pieces.bin_piece_off.data(), pieces.bin_piece_off.size()));
    t.seg_node = d_node;
    t.seg_starts = d_starts;
    t.seg_frac = d_frac;
    t.piece_off = d_piece_off;
    t.bin_piece_off = d_bin_piece_off;
    PML_TRY(mem.get(&t.partial, (size_t)cols * t.n_pieces * 3 * k));
    PML_TRY(mem.get(&t.xa, (size_t)cols * M * k));
    if (d_jumps != nullptr) {
        int *d_jpiece_off, *d_bin_jpiece_off;
        PML_TRY(mem.put(&d_jpiece_off, jpieces.piece_off.data(), jpieces.piece_off.size()));
        PML_TRY(mem.put(&d_bin_jpiece_off, jpieces.bin_piece_off.data(), jpieces.bin_piece_off.size()));
        t.jpiece_off = d_jpiece_off;
        t.bin_jpiece_off = d_bin_jpiece_off;
        PML_TRY(mem.get(&t.stage, (size_t)cols * t.n_segments * 3));
        PML_TRY(mem.get(&t.jpartial, (size_t)cols * t.n_jpieces * k * k));
    }
    if (t.n_pieces > 0) {
        const dim3 grid(t.n_pieces, cols);
        if (k <= 4) hipLaunchKernelGGL((history_time_segment_kernel<1, 4>), grid, dim3(256), 0, ctx->stream, t);
        else if (k <= 16) hipLaunchKernelGGL((history_time_segment_kernel<4, 4>), grid, dim3(256), 0, ctx->stream, t);
        else if (k <= 64) hipLaunchKernelGGL((history_time_segment_kernel<16, 4>), grid, dim3(256), 0, ctx->stream, t);
        else if (k <= 256) hipLaunchKernelGGL((history_time_segment_kernel<64, 4>), grid, dim3(256), 0, ctx->stream, t);
        else hipLaunchKernelGGL((history_time_segment_kernel<64, 8>), grid, dim3(256), 0, ctx->stream, t);
    }
    hipLaunchKernelGGL(history_time_vector_kernel, dim3(M + 1, cols), dim3(256), 0, ctx->stream, t);
    if (d_jumps != nullptr) {
        const int T = (k + 15) / 16, TG = (T + 3) / 4;
        if (t.n_jpieces > 0) {
            if (TG == 1) hipLaunchKernelGGL(history_time_jump_kernel<0>, dim3(t.n_jpieces, 1, cols), dim3(256), 0, ctx->stream, t);
            else hipLaunchKernelGGL(history_time_jump_kernel<1>, dim3(t.n_jpieces, TG * TG, cols), dim3(256), 0, ctx->stream, t);
        }
        hipLaunchKernelGGL(history_time_matrix_kernel, dim3(M * ((k * k + 255) / 256), cols), dim3(256), 0, ctx->stream, t);
    }
    HIP_TRY(hipGetLastError());
    return PML_OK;
}
