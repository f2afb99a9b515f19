// Launches of the exact dwell times, Markov jumps and lineage counts per time interval of the F81 family
// (pml_kernels_history_time.h): the segment pass, the jump product and the sums of the partials per bin, for the columns
// [cb, ce) of the context in one go, queued on the context's stream.  pml_history_through_time (pml_api_readers.hip) checks the
// arguments, plans the segments on the host (pml_time_segments.h), makes sure every vector the kernels read is in HBM and
// copies out.
#include "pml_launch.h"
#include "pml_kernels_history_time.h"

PML_INTERNAL int launch_history_time(pml_ctx* ctx, CallScope& mem, int cb, int ce, const PmlTimeSegments& plan, const PmlTimePieces& pieces,
                                     const PmlTimePieces& jpieces, double* d_times, double* d_jumps, double* d_lineages) {
    const int k = ctx->k, cols = ce - cb, M = plan.M;
    if (k > 512) return fail(PML_ERR_UNSUPPORTED, "k = %d: the F81 family holds at most 512 states", k);
    PmlHistTimeArgs t{};   // (what the jumps alone need stays null without them)
    history_args(ctx, cb, t.h);   // (its pieces stay 0: the pieces are the plan's, below)
    t.M = M;
    t.n_segments = plan.n_segments();
    t.n_pieces = pieces.n_pieces();
    t.n_jpieces = jpieces.n_pieces();
    t.times_out = d_times;
    t.jumps_out = d_jumps;
    t.lineages_out = d_lineages;
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
        with_branch_shape(k, [&](auto G, auto R) {
            hipLaunchKernelGGL((history_time_segment_kernel<G(), R()>), dim3(t.n_pieces, cols), dim3(256), 0, ctx->stream, t);
        });
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
