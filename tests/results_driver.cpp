// Host-only check of pastml_amd/csrc/pml_results.h: the record of what a context's result buffers hold, against a restatement
// of the loose fields of pml_ctx it replaced and of every place pml_api.hip wrote them (the commit before the record: one
// function per site, the site's assignments copied literally).  Every sequence of LENGTH entries of the library, with the
// boolean arguments of the sweeps enumerated, is played to both; after every step every query of the record must answer what
// the old fields answer.  Prints the number of sequences compared.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pastml_amd/csrc/pml_results.h"

static const int LENGTH = 4;

// ---- the fields as pml_ctx held them, and the sites that wrote them
struct Old {
    int bu_mode = -1;
    bool bu_fused = false, bu_absorbed = false, bu_fused_joint = false;
    bool td_valid = false, td_vec_valid = false, td_filled = false, tip_post_missing = false, post_ever = false;
    bool js_valid = false, js_ever = false;
    bool prep_dirty = true;
    bool active_partial = false;   // (read next to them; an input of the record)
};
// what the sites read from the rest of the context
struct Ctx {
    bool f81, cherries, super_sweeps, ran_batch;   // ran_batch: !sweep_without_p(ctx, is_marginal) && ctx->pij_window == 0
};

// pml_ctx_set_option, PML_OPT_EIGEN_FUSED
static void old_set_option_eigen_fused(Old& c) {
    c.prep_dirty = true;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
}
// pml_ctx_set_option, PML_OPT_EIGEN_JOINT_VALU
static void old_set_option_eigen_joint_valu(Old& c) {
    c.prep_dirty = true;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
}
// pml_ctx_set_tunable
static void old_set_tunable(Old& c) {
    c.prep_dirty = true;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
}
// pml_chars_alloc
static void old_chars_alloc(Old& c) {
    c.prep_dirty = true;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
}
// invalidate (pml_masks_upload, pml_masks_from_tip_states, set_common)
static void old_invalidate(Old& c) {
    c.prep_dirty = true;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
}
// pml_masks_initial_upload
static void old_masks_initial_upload(Old& c) { c.bu_mode = -1; }
// window_set
static void old_window_set(Old& c) { c.prep_dirty = true; }
// run_prep
static void old_run_prep(Old& c, bool force) {
    if (!c.prep_dirty && !force) return;
    c.prep_dirty = false;
}
// note_bottom_up
static void old_note_bottom_up(Old& c, const Ctx& x, bool is_marginal, bool fused_joint) {
    const bool f81_marginal = is_marginal && x.f81;
    c.js_valid = false;
    c.bu_fused_joint = fused_joint;
    if (x.ran_batch) c.prep_dirty = false;
    c.bu_fused = (f81_marginal && x.cherries) || c.bu_fused_joint;
    c.bu_absorbed = (f81_marginal && x.super_sweeps) || (c.active_partial && c.bu_absorbed);
}
// submit_bottom_up: set_active_columns, the reset before the sweep is enqueued, note_bottom_up once it is
static void old_submit_bottom_up(Old& c, const Ctx& x, bool is_marginal, bool partial, bool fused_joint, bool enqueued = true) {
    c.active_partial = partial;
    c.bu_mode = -1;
    c.td_valid = c.js_valid = false;
    if (!enqueued) return;
    old_note_bottom_up(c, x, is_marginal, fused_joint);
}
// collect_bottom_up, status == PML_OK
static void old_collect_bottom_up(Old& c, bool is_marginal) { c.bu_mode = is_marginal ? 1 : 0; }
// note_top_down (stored: ctx->kind != PML_MODEL_F81 || ctx->keep_td; implicit: state_of(ctx).implicit_tips)
static void old_note_top_down(Old& c, bool stored, bool implicit) {
    c.td_valid = true;
    c.td_vec_valid = stored;
    c.td_filled = false;
    c.post_ever = true;
    c.tip_post_missing = implicit;
}
// materialize_tip_posteriors
static void old_materialize_tip_posteriors(Old& c) {
    if (!c.tip_post_missing) return;
    c.tip_post_missing = false;
}
// materialize_cherries
static void old_materialize_cherries(Old& c) {
    if (c.bu_absorbed) c.bu_absorbed = false;
    if (!c.bu_fused) return;
    c.bu_fused = false;
}
// materialize_td (its top-down sweep runs with ctx->keep_td = true; force: ctx->d_P == nullptr || eigen_fused(ctx) || eigen_gemm(ctx))
static void old_materialize_td(Old& c, const Ctx& x, bool implicit, bool force) {
    if (!c.td_vec_valid) old_note_top_down(c, true, implicit);
    if (!c.td_filled) {
        if (x.f81) old_materialize_cherries(c);
        else old_run_prep(c, force);
        c.td_filled = true;
    }
}
// pml_top_down_marginals
static void old_top_down_marginals(Old& c, bool stored, bool implicit) {
    if (c.bu_mode != 1) return;   // refused
    old_note_top_down(c, stored, implicit);
}
// pml_marginal_pass; path 0: both sweeps enqueued, 1: captured as one graph just now, 2: that graph replayed
static void old_marginal_pass(Old& c, const Ctx& x, int path, bool stored, bool implicit, bool ok) {
    c.active_partial = false;   // set_active_columns(ctx, nullptr)
    if (path == 0) {
        old_submit_bottom_up(c, x, true, false, false);
        c.bu_mode = 1;  // provisional
        old_note_top_down(c, stored, implicit);
    } else {
        if (path == 1) {
            old_submit_bottom_up(c, x, true, false, false);
            c.bu_mode = 1;
            old_note_top_down(c, stored, implicit);
        }
        old_note_bottom_up(c, x, true, false);
        old_note_top_down(c, stored, implicit);
    }
    c.bu_mode = -1;
    if (ok) old_collect_bottom_up(c, true);
    else c.td_valid = false;
}
// fetch_joint_states
static void old_fetch_joint_states(Old& c) {
    c.js_valid = true;
    c.js_ever = true;
}
// pml_joint_backtrace
static void old_joint_backtrace(Old& c) {
    if (c.bu_mode != 0) return;   // refused
    old_fetch_joint_states(c);
}
// pml_joint_pass
static void old_joint_pass(Old& c, const Ctx& x, bool fused_joint, bool ok) {
    old_submit_bottom_up(c, x, false, false, fused_joint);
    old_fetch_joint_states(c);
    if (ok) old_collect_bottom_up(c, false);
    else c.js_valid = false;
}
// pml_select_states
static void old_select_states(Old& c) {
    if (!c.post_ever) return;   // refused
    old_materialize_tip_posteriors(c);
    c.prep_dirty = true;
    c.bu_mode = -1;
}
// download_internal, PML_BUF_TD
static void old_download_td(Old& c, const Ctx& x, bool implicit, bool force) {
    if (!c.td_valid) return;   // refused
    old_materialize_td(c, x, implicit, force);
}

// ---- the same entries as pml_api.hip plays them to the record
struct New {
    PmlResults r;
    bool active_partial = false;
};
static void new_run_prep(New& c, bool force) {
    if (!c.r.pij_stale() && !force) return;
    c.r.pij_built();
}
static void new_note_bottom_up(New& c, const Ctx& x, bool is_marginal, bool fused_joint) {
    c.r.bottom_up_submitted(is_marginal, x.f81, x.cherries, x.super_sweeps, x.ran_batch, c.active_partial, fused_joint);
}
static void new_materialize_tip_posteriors(New& c) {
    if (c.r.tip_posteriors_missing()) c.r.tip_posteriors_written();
}
static void new_materialize_cherries(New& c) {
    if (c.r.children_missing()) c.r.children_written();
    if (c.r.cherries_missing()) c.r.cherries_written();
}
static void new_marginal_pass(New& c, const Ctx& x, int path, bool stored, bool implicit, bool ok) {
    c.active_partial = false;
    for (int i = 0; i < (path == 1 ? 2 : 1); ++i) {   // (captured just now: once inside the capture, once behind run_captured)
        if (path != 2 && i == 0) c.r.no_results();    // submit_bottom_up, before the sweep is enqueued; a replay runs none
        new_note_bottom_up(c, x, true, false);
        c.r.top_down_submitted(stored, implicit);
    }
    if (ok) c.r.bottom_up_collected(true);
    else c.r.no_results();
}
static void new_joint_pass(New& c, const Ctx& x, bool fused_joint, bool ok) {
    c.active_partial = false;
    c.r.no_results();
    new_note_bottom_up(c, x, false, fused_joint);
    c.r.joint_states_fetched();
    if (ok) c.r.bottom_up_collected(false);
    else c.r.no_results();
}
static void new_download_td(New& c, const Ctx& x, bool implicit, bool force) {
    if (!c.r.has_top_down()) return;
    if (c.r.td_vectors_missing()) c.r.top_down_submitted(true, implicit);
    if (c.r.td_fill_missing()) {
        if (x.f81) new_materialize_cherries(c);
        else new_run_prep(c, force);
        c.r.td_fill_written();
    }
}

// ---- the alphabet: an entry and its arguments
enum Entry {
    SET_OPTION_EIGEN_FUSED, SET_OPTION_EIGEN_JOINT_VALU, SET_TUNABLE, CHARS_ALLOC, MASKS_OR_MODEL, MASKS_INITIAL, WINDOW_SET,
    RUN_PREP, SUBMIT, SUBMIT_FAILED, COLLECT, TOP_DOWN, MARGINAL_PASS, JOINT_BACKTRACE, JOINT_PASS, SELECT_STATES,
    MATERIALIZE_CHERRIES, MATERIALIZE_TIP_POSTERIORS, DOWNLOAD_TD, N_ENTRIES
};
struct Event {
    Entry entry;
    int path;       // MARGINAL_PASS
    bool a, b, c;   // the entry's booleans, in the order of its line in step()
};

static void step(Old& o, New& n, const Ctx& x, const Event& e) {
    switch (e.entry) {
        case SET_OPTION_EIGEN_FUSED: old_set_option_eigen_fused(o); n.r.inputs_changed(); break;
        case SET_OPTION_EIGEN_JOINT_VALU: old_set_option_eigen_joint_valu(o); n.r.inputs_changed(); break;
        case SET_TUNABLE: old_set_tunable(o); n.r.inputs_changed(); break;
        case CHARS_ALLOC: old_chars_alloc(o); n.r.inputs_changed(); break;
        case MASKS_OR_MODEL: old_invalidate(o); n.r.inputs_changed(); break;
        case MASKS_INITIAL: old_masks_initial_upload(o); n.r.initial_masks_changed(); break;
        case WINDOW_SET: old_window_set(o); n.r.pij_source_changed(); break;
        case RUN_PREP: old_run_prep(o, e.a); new_run_prep(n, e.a); break;
        case SUBMIT:   // a: marginal, b: some columns only, c: outcome.fused_joint
            old_submit_bottom_up(o, x, e.a, e.b, e.c);
            n.active_partial = e.b;
            n.r.no_results();
            new_note_bottom_up(n, x, e.a, e.c);
            break;
        case SUBMIT_FAILED:   // a: marginal, b: some columns only
            old_submit_bottom_up(o, x, e.a, e.b, false, false);
            n.active_partial = e.b;
            n.r.no_results();
            break;
        case COLLECT: old_collect_bottom_up(o, e.a); n.r.bottom_up_collected(e.a); break;
        case TOP_DOWN:   // a: TD vectors stored, b: observed tips implicit
            old_top_down_marginals(o, e.a, e.b);
            if (n.r.has_marginal()) n.r.top_down_submitted(e.a, e.b);
            break;
        case MARGINAL_PASS:   // a, b as TOP_DOWN; c: no zero likelihood
            old_marginal_pass(o, x, e.path, e.a, e.b, e.c);
            new_marginal_pass(n, x, e.path, e.a, e.b, e.c);
            break;
        case JOINT_BACKTRACE:
            old_joint_backtrace(o);
            if (n.r.has_joint()) n.r.joint_states_fetched();
            break;
        case JOINT_PASS:   // a: outcome.fused_joint, b: no zero likelihood
            old_joint_pass(o, x, e.a, e.b);
            new_joint_pass(n, x, e.a, e.b);
            break;
        case SELECT_STATES:
            old_select_states(o);
            if (n.r.posteriors_exist()) {
                new_materialize_tip_posteriors(n);
                n.r.masks_selected();
            }
            break;
        case MATERIALIZE_CHERRIES: old_materialize_cherries(o); new_materialize_cherries(n); break;
        case MATERIALIZE_TIP_POSTERIORS: old_materialize_tip_posteriors(o); new_materialize_tip_posteriors(n); break;
        case DOWNLOAD_TD: old_download_td(o, x, e.a, e.b); new_download_td(n, x, e.a, e.b); break;   // a: observed tips implicit, b: P(t) forced
        case N_ENTRIES: break;
    }
}

static std::vector<Event> alphabet() {
    static const int n_bools[N_ENTRIES] = {0, 0, 0, 0, 0, 0, 0, 1, 3, 2, 1, 2, 3, 0, 2, 0, 0, 0, 2};
    std::vector<Event> all;
    for (int entry = 0; entry < N_ENTRIES; ++entry)
        for (int path = 0; path < (entry == MARGINAL_PASS ? 3 : 1); ++path)
            for (int bits = 0; bits < (1 << n_bools[entry]); ++bits)
                all.push_back({(Entry)entry, path, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0});
    return all;
}

static const char* differ(const Old& o, const New& n) {
    const PmlResults& r = n.r;
    if (r.has_marginal() != (o.bu_mode == 1)) return "has_marginal";
    if (r.has_joint() != (o.bu_mode == 0)) return "has_joint";
    if (r.has_bottom_up() != (o.bu_mode >= 0)) return "has_bottom_up";
    if (r.has_top_down() != o.td_valid) return "has_top_down";
    if (r.has_joint_states() != o.js_valid) return "has_joint_states";
    if (r.posteriors_exist() != o.post_ever) return "posteriors_exist";
    if (r.joint_states_exist() != o.js_ever) return "joint_states_exist";
    if (r.pij_stale() != o.prep_dirty) return "pij_stale";
    if (r.cherries_missing() != o.bu_fused) return "cherries_missing";
    if (r.cherries_joint() != o.bu_fused_joint) return "cherries_joint";
    if (r.children_missing() != o.bu_absorbed) return "children_missing";
    if (r.td_vectors_missing() != !o.td_vec_valid) return "td_vectors_missing";
    if (r.td_fill_missing() != !o.td_filled) return "td_fill_missing";
    if (r.tip_posteriors_missing() != o.tip_post_missing) return "tip_posteriors_missing";
    if (n.active_partial != o.active_partial) return "active_partial";
    // the two invariants, on their own
    if (r.has_top_down() && !r.posteriors_exist()) return "has_top_down without posteriors";
    if (r.has_joint_states() && !r.joint_states_exist()) return "has_joint_states without joint states";
    return nullptr;
}

static const std::vector<Event> kEvents = alphabet();
static long long n_sequences = 0;
static int trail[LENGTH];

static void walk(const Old& o, const New& n, const Ctx& x, int depth) {
    if (depth == LENGTH) {
        ++n_sequences;
        return;
    }
    for (size_t i = 0; i < kEvents.size(); ++i) {
        Old o2 = o;
        New n2 = n;
        trail[depth] = (int)i;
        step(o2, n2, x, kEvents[i]);
        if (const char* what = differ(o2, n2)) {
            printf("FAIL: %s differs (f81 %d cherries %d two-level %d batch %d) after", what, x.f81, x.cherries, x.super_sweeps, x.ran_batch);
            for (int d = 0; d <= depth; ++d) {
                const Event& e = kEvents[trail[d]];
                printf(" [entry %d path %d %d%d%d]", (int)e.entry, e.path, e.a, e.b, e.c);
            }
            printf("\n");
            exit(1);
        }
        walk(o2, n2, x, depth + 1);
    }
}

int main() {
    if (differ(Old(), New())) {
        printf("FAIL: a fresh record differs from fresh fields\n");
        return 1;
    }
    for (int cfg = 0; cfg < 16; ++cfg) {
        const Ctx x = {(cfg & 1) != 0, (cfg & 2) != 0, (cfg & 4) != 0, (cfg & 8) != 0};
        walk(Old(), New(), x, 0);
    }
    printf("OK: %lld sequences of %d entries (%zu entries with their arguments, 16 kinds of context), every query after every step\n",
           n_sequences, LENGTH, kEvents.size());
    return 0;
}
