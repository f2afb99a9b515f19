// The entries of the C-ABI (include/pastml_hip.h) that read what a marginal pass left on the device -- and pml_simulate_states,
// which reads the model alone.  They have one shape: check the arguments; make sure a marginal pass has run (Reader::pass) and
// that every row of it is in HBM, on an idle stream (Reader::rows); take the outputs and the scratch from a CallScope
// (pml_call_scope.h), each output's size written once (CallScope::out); call one launch_* (pml_launch.h); copy out and wait
// (CallScope::finish).  What two of them share stands here once.  The entry's own refusals sit between the steps, where they
// always sat: which of two refusals a caller sees is behaviour (tests/test_gpu_reader_refusals.py).  Nothing here touches the
// sweeps, their plans or their graphs: those are pml_api.hip's, which also defines the helpers declared at the end of pml_host.h.
#include "pml_launch.h"

namespace {   // what the entries share

// What an entry asks of the context.  columns(), pass() and rows() run in this order, the entry's own refusals between them.
struct Reader {
    pml_ctx* ctx;
    const char* entry;                // who asks (the messages name it)
    int cb, ce;                       // the columns it reads
    const char* f81_what = nullptr;   // set: an entry of the F81 family, which computes this; null: any model kind
    int f81_most = 0;                 // ... and holds at most this many states (0: no bound of its own)
    bool idle = true;                 // rows() waits for an idle stream first
    bool prep = true;                 // the rows include P(t) / exp(-mu t') of every branch (or the window's parameters)

    // a model in every column, and the range within them
    int columns() const {
        PML_TRY(require_model(ctx));
        return check_cols(ctx, cb, ce);
    }
    // the results of a marginal bottom-up and a top-down sweep; ahead of them, for the F81 family: the bound on the states and
    // that model kind -- then two states or more, and a finite positive mu in every column of [cb, ce)
    int pass() const {
        if (f81_most > 0 && ctx->k > f81_most)
            return fail(PML_ERR_UNSUPPORTED, "%s: k = %d, the F81 family holds at most %d states", entry, ctx->k, f81_most);
        if (f81_what != nullptr && ctx->kind != PML_MODEL_F81)
            return fail(PML_ERR_UNSUPPORTED, "%s is for the F81 family (F81, JC, EFT): this context's model kind is %s", entry,
                        ctx->kind == PML_MODEL_HKY ? "HKY" : "eigen");
        if (!ctx->results.has_marginal() || !ctx->results.has_top_down())
            return fail(PML_ERR_INVALID, "%s needs a marginal pml_bottom_up and pml_top_down_marginals first", entry);
        if (f81_what == nullptr) return PML_OK;
        if (ctx->k < 2) return fail(PML_ERR_INVALID, "%s: k = %d, a character of one state has no %s", entry, ctx->k, f81_what);
        const double* mu = ctx->h_params + ctx->cols.params.mu;
        for (int c = cb; c < ce; ++c)
            if (!std::isfinite(mu[c]) || !(mu[c] > 0.0))
                return fail(PML_ERR_INVALID, "%s: column %d has pi . pi >= 1 (mu is not finite)", entry, c);
        return PML_OK;
    }
    // every row of the pass in memory (once the entry knows that it holds this many states: the batch is allocated here)
    int rows() const {
        if (idle) PML_TRY(wait_pending(ctx, true));   // (a pass that ended in a spin on the completion word may have left the stream busy)
        PML_TRY(materialize_cherries(ctx));          // the conditional probabilities need every bottom-up vector
        PML_TRY(materialize_tip_posteriors(ctx));    // (a single-tip tree's root; the rows of the scenario sampler's fallback)
        // P(t) of every branch (the fused sweeps never materialise it) / exp(-mu t'); or the window
        return prep ? consumer_prep(ctx) : PML_OK;
    }
};

// The arguments of an entry that draws n_repetitions of column col, refused in this order: the column or an output the entry
// cannot do without; `also`, a refusal of the entry's own that ranks here (or null); n_repetitions; rep_offset.  prefix: what
// the entry's messages begin with.
static int check_draws(const pml_ctx* ctx, const char* prefix, int col, bool outputs, const char* also, int n_repetitions,
                       int rep_offset) {
    if (col < 0 || col >= ctx->C || !outputs) return fail(PML_ERR_INVALID, "%sbad column / output", prefix);
    if (also != nullptr) return fail(PML_ERR_INVALID, "%s%s", prefix, also);
    if (n_repetitions <= 0) return fail(PML_ERR_INVALID, "%sn_repetitions must be positive", prefix);
    if (rep_offset < 0) return fail(PML_ERR_INVALID, "%srep_offset must not be negative", prefix);
    return PML_OK;
}

// The states of n_rep repetitions per node on the device, in the caller's numbering: one byte per state up to 256 states, two
// beyond; rows padded to a multiple of 4 repetitions and copied out without the padding.
struct StateRows {
    size_t n_rep, es, rs;
    unsigned char* d = nullptr;
    StateRows(const pml_ctx* ctx, int n_repetitions) : n_rep((size_t)n_repetitions), es(ctx->k > 256 ? 2 : 1), rs((n_rep + 3) / 4 * 4) {}
    int alloc(const pml_ctx* ctx, CallScope& mem) { return mem.get(&d, (size_t)ctx->N * rs * es); }
    int copy_out(const pml_ctx* ctx, void* states_out) const {
        if (states_out != nullptr)
            HIP_TRY(hipMemcpy2DAsync(states_out, n_rep * es, d, rs * es, n_rep * es, (size_t)ctx->N, hipMemcpyDeviceToHost, ctx->stream));
        return PML_OK;
    }
};

// The two counters of the history samplers: the scenarios' fallbacks, the branches not drawn.  Declared before the scope.
struct HistoryCounters {
    unsigned long long host[2] = {0, 0};
    unsigned long long* d = nullptr;
    int alloc(CallScope& mem) { return mem.out(&d, host, 2, true); }
    // (behind the scope's wait)
    int report(const char* entry, int64_t* n_fallback_out) const {
        *n_fallback_out = (int64_t)host[0];
        if (host[1])
            return fail(PML_ERR_UNSUPPORTED, "%s: %llu branches have x = mu t' > 512 (PML_HSAMP_MAX_X), where exp(-x) leaves the "
                        "normal doubles: they were not drawn and the outputs are not histories", entry, host[1]);
        return PML_OK;
    }
};

// The segment plan of a time entry (pml_time_segments.h), made on the host and in the caller's numbering -- it does not depend
// on the column.  what: whose size M k^2 bounds in the call's scratch.
static int plan_time_segments(const pml_ctx* ctx, const char* entry, const char* what, const double* node_time, const double* boundaries,
                              int M, PmlTimeSegments& plan) {
    const long long cells = (long long)M * ctx->k * ctx->k;
    if (M >= 1 && cells > (long long)PML_HIST_TIME_MAX_CELLS)
        return fail(PML_ERR_UNSUPPORTED, "%s: M k^2 = %lld is beyond %d (PML_HIST_TIME_MAX_CELLS): %s would not fit the call's scratch; "
                    "ask for fewer bins per call", entry, cells, PML_HIST_TIME_MAX_CELLS, what);
    const size_t N = (size_t)ctx->N;
    std::vector<int> parent(N);   // the caller's numbering
    const bool same = ctx->new_of_old.empty();
    for (size_t i = 0; i < N; ++i) {
        const int p = ctx->forest.parent[same ? i : (size_t)ctx->new_of_old[i]];
        parent[i] = (p < 0 || same) ? p : ctx->old_of_new[p];
    }
    const std::string why = pml_plan_time_segments(parent.data(), node_time, (int)N, boundaries, M, plan);
    if (!why.empty()) return fail(PML_ERR_INVALID, "%s: %s", entry, why.c_str());
    return PML_OK;
}

// The outputs of the two exact histories of the columns [cb, ce), and the launch that fills them: times [cols][k], jumps
// [cols][k][k] or null, the jumps per branch [cols][N] or null.
static int history_outputs(pml_ctx* ctx, decltype(launch_history)* launch, int cb, int ce, double* times_out, double* jumps_out,
                           double* branch_jumps_out) {
    const size_t k = ctx->k, N = (size_t)ctx->N, cols = (size_t)(ce - cb);
    CallScope mem(ctx->stream, false);
    double *d_times, *d_jumps, *d_branch;
    PML_TRY(mem.out(&d_times, times_out, cols * k));
    PML_TRY(mem.out(&d_jumps, jumps_out, cols * k * k));
    PML_TRY(mem.out(&d_branch, branch_jumps_out, cols * N));
    PML_TRY(launch(ctx, mem, cb, ce, d_times, d_jumps, d_branch));
    return mem.finish();
}

// What the two histories of the eigen-decomposed models refuse, each in its place.  eigen_kind: an F81 context (f81_entry serves
// it), an HKY context; eigen_states: fewer than 2 or more than 256 states; eigen_columns: a column of [cb, ce) whose scaling factor
// is not finite and positive or whose eigenvalues are not finite.
static int eigen_kind(const pml_ctx* ctx, const char* entry, const char* f81_entry) {
    if (ctx->kind == PML_MODEL_F81)
        return fail(PML_ERR_UNSUPPORTED, "%s is for the eigen-decomposed models: this context's model kind is F81 (F81, JC, EFT), "
                    "which %s serves", entry, f81_entry);
    if (ctx->kind == PML_MODEL_HKY)
        return fail(PML_ERR_UNSUPPORTED, "%s is for the eigen-decomposed models: this context's model kind is HKY; hand the model "
                    "over as an eigen model (pml_model_set_eigen with the d, A, Ainv of its rate matrix)", entry);
    return PML_OK;
}
static int eigen_states(const pml_ctx* ctx, const char* entry) {
    if (ctx->k < 2) return fail(PML_ERR_INVALID, "%s: k = %d, a character of one state has no history", entry, ctx->k);
    if (ctx->k > 256) return fail(PML_ERR_UNSUPPORTED, "%s: k = %d, the matrix models hold at most 256 states", entry, ctx->k);
    return PML_OK;
}
static int eigen_columns(const pml_ctx* ctx, const char* entry, int cb, int ce) {
    const size_t k = ctx->k;
    const double* sf = ctx->h_params + ctx->cols.params.sf;
    for (int c = cb; c < ce; ++c) {
        if (!std::isfinite(sf[c]) || !(sf[c] > 0.0))
            return fail(PML_ERR_INVALID, "%s: column %d has a scaling factor that is not finite and positive", entry, c);
        for (size_t m = 0; m < k; ++m)
            if (ctx->h_eig_d.size() != (size_t)ctx->C * k || !std::isfinite(ctx->h_eig_d[(size_t)c * k + m]))
                return fail(PML_ERR_INVALID, "%s: column %d has an eigenvalue that is not finite", entry, c);
    }
    return PML_OK;
}

}   // namespace

// altered (caller's ids, or null): see counts_level_kernel.  result_out: the k x k sums of the draws (not divided by
// n_repetitions when altered is given); state_counts_out / same_out: [N][k] in the caller's numbering.  (The one reader of a pass
// that does not wait for an idle stream before it writes the rows.)
static int marginal_counts_impl(pml_ctx* ctx, int32_t col, int32_t n_repetitions, uint64_t seed, const uint8_t* altered,
                                double* result_out, int32_t* state_counts_out, int32_t* same_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(check_draws(ctx, "", col, result_out != nullptr, nullptr, n_repetitions, 0));
    const Reader r = {ctx, "pml_marginal_counts", col, col + 1, nullptr, 0, false};
    PML_TRY(r.pass());
    if (ctx->k > counts_max_states()) return fail(PML_ERR_UNSUPPORTED, "k = %d: at most %d states", ctx->k, counts_max_states());
    PML_TRY(r.rows());
    const size_t k = ctx->k, per_node = (size_t)ctx->N * k;
    std::vector<unsigned char> alt;
    std::vector<long long> h(k * k);
    CallScope mem(ctx->stream, false);
    int *d_counts, *d_same = nullptr;
    long long* d_result;
    unsigned char* d_alt = nullptr;
    PML_TRY(mem.get(&d_counts, per_node));
    PML_TRY(mem.out(&d_result, h.data(), h.size(), true));
    if (altered != nullptr) {
        PML_TRY(upload_altered(ctx, mem, altered, alt, &d_alt));
        PML_TRY(mem.get(&d_same, per_node));
        HIP_TRY(hipMemsetAsync(d_same, 0, per_node * sizeof(int), ctx->stream));
    }
    PML_TRY(launch_counts(ctx, col, n_repetitions, seed, d_alt, d_counts, d_result, d_same));
    if (altered != nullptr) {
        // (tips' rows of d_counts are written by their parents' passes: every node has its row)
        PML_TRY(fetch_rows(ctx, d_counts, k, k, 1, state_counts_out));
        PML_TRY(fetch_rows(ctx, d_same, k, k, 1, same_out));
    }
    PML_TRY(mem.finish());
    for (size_t i = 0; i < h.size(); ++i) result_out[i] = altered != nullptr ? (double)h[i] : (double)h[i] / (double)n_repetitions;
    return PML_OK;
}

int pml_marginal_counts(pml_ctx* ctx, int32_t col, int32_t n_repetitions, uint64_t seed, double* counts_out) {
    return marginal_counts_impl(ctx, col, n_repetitions, seed, nullptr, counts_out, nullptr, nullptr);
}

int pml_marginal_counts_altered(pml_ctx* ctx, int32_t col, int32_t n_repetitions, uint64_t seed, const uint8_t* altered,
                                double* sums_out, int32_t* state_counts_out, int32_t* same_out) {
    if (!altered || !state_counts_out || !same_out) return fail(PML_ERR_INVALID, "NULL array");
    return marginal_counts_impl(ctx, col, n_repetitions, seed, altered, sums_out, state_counts_out, same_out);
}

// Exact expected transition counts of the columns [col_begin, col_end) (pml_launch_expected.hip): the limit of the sampler above
// for n_repetitions -> infinity, from the vectors the marginal pass left on the device.  altered (caller's ids, or null): the
// pairs with an altered end are left out and their parents' same-state sums go to same_out, as in pml_marginal_counts_altered.
int pml_expected_counts(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint8_t* altered, double* counts_out,
                        double* same_out) {
    const Reader r = {ctx, "pml_expected_counts", col_begin, col_end};
    PML_TRY(r.columns());
    if (!counts_out) return fail(PML_ERR_INVALID, "counts_out is NULL");
    PML_TRY(r.pass());
    if (ctx->kind != PML_MODEL_F81 && ctx->k > 256)
        return fail(PML_ERR_UNSUPPORTED, "k = %d: the matrix models hold at most 256 states", ctx->k);
    PML_TRY(r.rows());
    const size_t k = ctx->k, N = (size_t)ctx->N, cols = (size_t)(col_end - col_begin);
    std::vector<unsigned char> alt;
    CallScope mem(ctx->stream, false);
    double *d_out, *d_same;
    unsigned char* d_alt = nullptr;
    PML_TRY(mem.out(&d_out, counts_out, cols * k * k));
    if (altered != nullptr) PML_TRY(upload_altered(ctx, mem, altered, alt, &d_alt));
    PML_TRY(mem.out(&d_same, altered != nullptr ? same_out : nullptr, cols * N * k, true));
    PML_TRY(launch_expected(ctx, col_begin, col_end, d_alt, d_out, d_same));
    return mem.finish();
}

// Exact gradient of ln L of the columns [col_begin, col_end) under the F81 family (pml_launch_gradient.hip): one streaming pass
// over the vectors the marginal pass left on the device, no sweep.  The masks are those the pass ran with.
int pml_loglik_gradient(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* d_rates_out, double* d_pi_out,
                        int32_t* n_flat_out) {
    const Reader r = {ctx, "pml_loglik_gradient", col_begin, col_end, "gradient"};
    PML_TRY(r.columns());
    if (!d_rates_out || !d_pi_out || !n_flat_out) return fail(PML_ERR_INVALID, "pml_loglik_gradient: an output array is NULL");
    PML_TRY(r.pass());
    PML_TRY(r.rows());
    const size_t k = ctx->k, cols = (size_t)(col_end - col_begin);
    CallScope mem(ctx->stream, false);
    double *d_rates, *d_pi;
    int* d_flat;
    PML_TRY(mem.out(&d_rates, d_rates_out, cols * 3));
    PML_TRY(mem.out(&d_pi, d_pi_out, cols * k));
    PML_TRY(mem.out(&d_flat, n_flat_out, cols));
    PML_TRY(launch_gradient(ctx, mem, col_begin, col_end, d_rates, d_pi, d_flat));
    return mem.finish();
}

// Exact expected dwell times and Markov jumps of the columns [col_begin, col_end) under the F81 family (pml_launch_history.hip):
// one streaming pass over the vectors the marginal pass left on the device, and the jump product where jumps_out is given.  The
// masks are those the pass ran with.
int pml_expected_history(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* times_out, double* jumps_out,
                         double* branch_jumps_out) {
    const Reader r = {ctx, "pml_expected_history", col_begin, col_end, "history", 512};
    PML_TRY(r.columns());
    if (!times_out) return fail(PML_ERR_INVALID, "pml_expected_history: times_out is NULL");
    PML_TRY(r.pass());
    PML_TRY(r.rows());
    return history_outputs(ctx, launch_history, col_begin, col_end, times_out, jumps_out, branch_jumps_out);
}

// Exact expected dwell times and Markov jumps of the columns [col_begin, col_end) under the eigen-decomposed models
// (pml_launch_history_eigen.hip): the eigenbasis integral over the vectors the marginal pass left on the device.  No P(t): the
// bottom-up vectors and the posteriors are made complete, the batch (or the window) is not touched.  The masks are those the pass
// ran with.
int pml_expected_history_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* times_out, double* jumps_out,
                               double* branch_jumps_out) {
    const Reader r = {ctx, "pml_expected_history_eigen", col_begin, col_end, nullptr, 0, true, false};
    const char* entry = r.entry;
    PML_TRY(r.columns());
    if (!times_out) return fail(PML_ERR_INVALID, "%s: times_out is NULL", entry);
    PML_TRY(eigen_kind(ctx, entry, "pml_expected_history"));
    PML_TRY(r.pass());
    PML_TRY(eigen_states(ctx, entry));
    PML_TRY(eigen_columns(ctx, entry, col_begin, col_end));
    PML_TRY(r.rows());
    return history_outputs(ctx, launch_history_eigen, col_begin, col_end, times_out, jumps_out, branch_jumps_out);
}

// The same per time interval, with the lineages at every boundary (pml_launch_history_time.hip).  The segment plan is uploaded
// through the call's scope; plan and pieces are declared before the scope, whose wait ends the copies that read them.
int pml_history_through_time(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* node_time, const double* boundaries,
                             int32_t M, double* times_out, double* jumps_out, double* lineages_out) {
    const Reader r = {ctx, "pml_history_through_time", col_begin, col_end, "history", 512};
    PML_TRY(r.columns());
    if (!times_out || !node_time || !boundaries)
        return fail(PML_ERR_INVALID, "pml_history_through_time: node_time, boundaries or times_out is NULL");
    PML_TRY(r.pass());
    PmlTimeSegments plan;
    PmlTimePieces pieces, jpieces;
    PML_TRY(plan_time_segments(ctx, r.entry, "the partials of the bins", node_time, boundaries, M, plan));
    pieces = pml_cut_time_pieces(plan, history_piece(ctx->k), true);
    if (jumps_out) jpieces = pml_cut_time_pieces(plan, history_jump_piece(ctx->k), false);
    PML_TRY(r.rows());
    const size_t k = ctx->k, cols = (size_t)(col_end - col_begin), bins = (size_t)M;
    CallScope mem(ctx->stream, false);
    double *d_times, *d_jumps, *d_lineages;
    PML_TRY(mem.out(&d_times, times_out, cols * bins * k));
    PML_TRY(mem.out(&d_jumps, jumps_out, cols * bins * k * k));
    PML_TRY(mem.out(&d_lineages, lineages_out, cols * (bins + 1) * k));
    PML_TRY(launch_history_time(ctx, mem, col_begin, col_end, plan, pieces, jpieces, d_times, d_jumps, d_lineages));
    return mem.finish();
}

// The same per time interval, with the lineages at every boundary (pml_launch_history_time_eigen.hip): pml_history_through_time
// for the eigen-decomposed models.  The plan and what is derived from it are declared before the scope, whose wait ends the copies
// that read them.
int pml_history_through_time_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* node_time, const double* boundaries,
                                   int32_t M, double* times_out, double* jumps_out, double* lineages_out) {
    const Reader r = {ctx, "pml_history_through_time_eigen", col_begin, col_end, nullptr, 0, true, false};
    const char* entry = r.entry;
    PML_TRY(r.columns());
    if (!times_out || !node_time || !boundaries) return fail(PML_ERR_INVALID, "%s: node_time, boundaries or times_out is NULL", entry);
    PML_TRY(eigen_kind(ctx, entry, "pml_history_through_time"));
    PML_TRY(r.pass());
    PML_TRY(eigen_states(ctx, entry));
    HistoryTimeEigenPlan host;
    PML_TRY(plan_time_segments(ctx, entry, "the sums of the bins", node_time, boundaries, M, host.plan));
    PML_TRY(eigen_columns(ctx, entry, col_begin, col_end));
    history_time_eigen_plan(host);
    PML_TRY(r.rows());
    const size_t k = ctx->k, cols = (size_t)(col_end - col_begin), bins = (size_t)M;
    CallScope mem(ctx->stream, false);
    double *d_times, *d_jumps, *d_lineages;
    PML_TRY(mem.out(&d_times, times_out, cols * bins * k));
    PML_TRY(mem.out(&d_jumps, jumps_out, cols * bins * k * k));
    PML_TRY(mem.out(&d_lineages, lineages_out, cols * (bins + 1) * k));
    PML_TRY(launch_history_time_eigen(ctx, mem, col_begin, col_end, host, d_times, d_jumps, d_lineages));
    return mem.finish();
}

// n_repetitions scenarios of column col drawn forward from the roots (pml_launch_simulate.hip).  Needs a model, no sweep -- hence
// no Reader --: the per-branch e = exp(-mu t') (F81 family) or P(t) is prepared here, and nothing waits for the stream first.
int pml_simulate_states(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed, void* states_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(check_draws(ctx, "", col, states_out != nullptr, nullptr, n_repetitions, rep_offset));
    // (the sweeps may have left E / P(t) in registers only, or for other parameters: prepared afresh; a context with a window
    // pushes the parameters and builds its matrices run by run)
    PML_TRY(window_from_tunable(ctx));
    PML_TRY(consumer_prep(ctx, true));
    StateRows states(ctx, n_repetitions);
    CallScope mem(ctx->stream, false);
    PML_TRY(states.alloc(ctx, mem));
    PML_TRY(launch_simulate(ctx, col, rep_offset, seed, states.d, states.rs));
    PML_TRY(states.copy_out(ctx, states_out));
    return mem.finish();
}

// n_repetitions scenarios of column col drawn from the joint posterior (pml_launch_scenarios.hip), from the vectors the marginal
// pass left on the device.  n_fallback_out: the draws that found no weight.
int pml_sample_scenarios(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed, void* states_out,
                         int64_t* n_fallback_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(check_draws(ctx, "", col, states_out && n_fallback_out, nullptr, n_repetitions, rep_offset));
    const Reader r = {ctx, "pml_sample_scenarios", col, col + 1};
    PML_TRY(r.pass());
    const int most = ctx->kind == PML_MODEL_F81 ? 512 : 256;
    if (ctx->k > most) return fail(PML_ERR_UNSUPPORTED, "k = %d: pml_sample_scenarios holds at most %d states for this model", ctx->k, most);
    PML_TRY(r.rows());
    StateRows states(ctx, n_repetitions);
    unsigned long long fallen = 0;
    CallScope mem(ctx->stream, false);
    unsigned long long* d_fallen;
    PML_TRY(states.alloc(ctx, mem));
    PML_TRY(mem.out(&d_fallen, &fallen, 1, true));
    PML_TRY(launch_scenarios(ctx, col, n_repetitions, rep_offset, seed, states.d, states.rs, d_fallen));
    PML_TRY(states.copy_out(ctx, states_out));
    PML_TRY(mem.finish());
    *n_fallback_out = (int64_t)fallen;
    return PML_OK;
}

// n_repetitions histories of column col under the F81 family (pml_launch_history_sample.hip): the scenarios of
// pml_sample_scenarios, written to a device buffer in the same call (the same seed, the same bits; they go through the host only
// if states_out asks for them), then on every branch the events between its two end states.
int pml_sample_histories(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed, void* states_out,
                         double* times_out, uint32_t* jumps_out, uint16_t* branch_jumps_out, int64_t* n_fallback_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(check_draws(ctx, "pml_sample_histories: ", col, times_out && n_fallback_out, nullptr, n_repetitions, rep_offset));
    const Reader r = {ctx, "pml_sample_histories", col, col + 1, "history", 512};
    PML_TRY(r.pass());
    PML_TRY(r.rows());
    const size_t k = ctx->k, N = (size_t)ctx->N, R = (size_t)n_repetitions;
    StateRows states(ctx, n_repetitions);
    HistoryCounters counters;
    CallScope mem(ctx->stream, false);
    double* d_times;
    unsigned* d_jumps;
    unsigned short* d_branch;
    PML_TRY(states.alloc(ctx, mem));
    PML_TRY(mem.out(&d_times, times_out, R * k));
    PML_TRY(mem.out(&d_jumps, jumps_out, R * k * k, true));
    PML_TRY(mem.out(&d_branch, branch_jumps_out, N * R));
    PML_TRY(counters.alloc(mem));
    PML_TRY(launch_scenarios(ctx, col, n_repetitions, rep_offset, seed, states.d, states.rs, counters.d));
    PML_TRY(launch_history_sample(ctx, mem, col, n_repetitions, rep_offset, seed, states.d, states.rs, d_times, d_jumps, d_branch,
                                  counters.d + 1));
    PML_TRY(states.copy_out(ctx, states_out));
    PML_TRY(mem.finish());
    return counters.report(r.entry, n_fallback_out);
}

// The same histories cut at the boundaries of M time bins (pml_launch_history_time_sample.hip): the scenarios as above, the
// segment plan of pml_history_through_time with its upper ends.  The plan and the tables derived from it are declared before the
// scope, whose wait ends the copies that read them.
int pml_sample_histories_through_time(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed,
                                      const double* node_time, const double* boundaries, int32_t M, void* states_out,
                                      double* times_out, uint32_t* jumps_out, uint32_t* lineages_out, int64_t* n_fallback_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(check_draws(ctx, "pml_sample_histories_through_time: ", col, times_out && n_fallback_out,
                        !node_time || !boundaries ? "node_time or boundaries is NULL" : nullptr, n_repetitions, rep_offset));
    const Reader r = {ctx, "pml_sample_histories_through_time", col, col + 1, "history", 512};
    PML_TRY(r.pass());
    HistoryTimeSamplePlan host;
    PML_TRY(plan_time_segments(ctx, r.entry, "the jump tables of a repetition", node_time, boundaries, M, host.plan));
    host.ends = pml_time_segment_ends(host.plan);
    host.pieces = pml_cut_time_pieces(host.plan, history_time_sample_piece(ctx->N), lineages_out != nullptr);
    PML_TRY(r.rows());
    const size_t k = ctx->k, R = (size_t)n_repetitions, bins = (size_t)M;
    StateRows states(ctx, n_repetitions);
    HistoryCounters counters;
    CallScope mem(ctx->stream, false);
    double* d_times;
    unsigned *d_jumps, *d_lineages;
    PML_TRY(states.alloc(ctx, mem));
    PML_TRY(mem.out(&d_times, times_out, R * bins * k));
    PML_TRY(mem.out(&d_jumps, jumps_out, R * bins * k * k, true));
    PML_TRY(mem.out(&d_lineages, lineages_out, R * (bins + 1) * k, true));
    PML_TRY(counters.alloc(mem));
    PML_TRY(launch_history_time_sample(ctx, mem, col, n_repetitions, rep_offset, seed, states.d, states.rs, host, d_times, d_jumps,
                                       d_lineages, counters.d, counters.d + 1));
    PML_TRY(states.copy_out(ctx, states_out));
    PML_TRY(mem.finish());
    return counters.report(r.entry, n_fallback_out);
}
